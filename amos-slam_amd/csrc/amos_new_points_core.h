// amos_new_points_core.h -- what LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:313-626) computes between its search and its
// `new MapPoint`, written once for host and device: pair_geometry (ComputeF12 :743-779, the epipole of ORBmatcher.cc:818-825 and the
// stereo / RGB-D baseline gate :361-374) and triangulate_match (:424-597 for one match: the parallax of the two rays, the 4 x 4 SVD or
// KeyFrame::UnprojectStereo (KeyFrame.cc:805-830), the two depth signs, the two reprojection gates, the scale-consistency gate).
// Included by amos_new_points.hip (k_new_points_solve: one match per lane; amos_kf_geometry_from_poses: the host compilation inside the
// library); tests/host_new_points compiles it as plain C++ into a complete host loop.  tests/new_points_restatement.py is the same
// arithmetic in numpy float32 / float64 and the tests hold both compilations to it bit for bit: every operation is rounded on its own, in
// source order (explicit _rn operations on the device, -ffp-contract=off on the host), library functions are restated with + - * / sqrt.
// PARITY WITH THE REFERENCE'S OPENCV-BACKED ARITHMETIC IS UNPINNED (cv::SVD runs in float, cv::Mat::inv, cos and atan2 are library code).
// The monocular median-depth gate (:375-385) is OUT OF SCOPE: the product is RGB-D, mbMonocular is false.
// The conventions that fix each expression (the cv::Mat ones are those of amos_sim3_core.h and host/ORBmatcher_adaptors.h, restated):
//   A * B, A * B + C               one gemm: the products widened to double and summed left to right, C added in double, ONE rounding
//                                  to float (R1w * R2w.t(), Rwc * xn, Twc.R * x3Dc + Twc.t, the three products of F12)
//   -A * B' * c + d (t12, :767)    the first product is a matrix of its own: (float) -(the double sum), which is -R12 exactly; then ONE
//                                  gemm with d added in double
//   K.inv(), K.t().inv()           the closed form for a pinhole K: [invfx 0 -cx*invfx; 0 invfy -cy*invfy; 0 0 1] with float32 products,
//                                  invfx and invfy the keyframe's own members; the transpose of the same entries
//   Mat::dot (:475, :508-..)       a double accumulator from 0.0 over the float32 products, left to right (amos_sim3_core.h)
//   cv::norm                       sqrt in double of the double products of the float32 entries summed left to right (amos_adapt::norm)
//   dot / (norm * norm), dot + t   in double, ONE rounding to float where the reference assigns a float
//   s * row - row (A, :486-489)    float32: one product, one difference per entry
//   cos(2 * atan2(mb / 2, d))      (d^2 - h^2) / (d^2 + h^2) in double from the float32 d and h = mb / 2 (a float32 quotient), ONE rounding
//                                  to float; 1 when both are 0.  With t = atan2(h, d) and r = sqrt(d^2 + h^2) > 0, cos t = d / r and
//                                  sin t = h / r in every quadrant (that is atan2's definition), and cos 2t = cos^2 t - sin^2 t.
//   cv::SVD::compute(A), vt.row(3) AtA = A^T A in double from the sixteen float32 entries (each sum over the rows in order), jacobi_sym4 (the
//                                  4 x 4 form of pnp::jacobi_sym, the same operations in the same order), the eigenvector of the SMALLEST
//                                  eigenvalue, the first of equal ones (pnp::eig_order ascending), each component rounded to float
//   x3D / w                        one float32 product per component with (float)(1.0 / (double) w) (the A / s rule)
//   1.0 / z                        invz = (float)(1.0 / (double) z)
//   e > 5.991 * sigma2, 7.8        (double) e against the double product
//   the scale test (:596)          float32 throughout, ratioFactor = 1.5f * scale_factor
//   UnprojectStereo                (u - cx) * z * invfx left to right in float32 from the RAW keypoint (mvKeys, KeyFrame.cc:816-817)
// The reference's own quirks are behaviour and are kept: `else if (bStereo2)` at :458 (with both features stereo only cosParallaxStereo1
// is computed), the CURRENT keyframe's mbf in keyframe 2's stereo reprojection (:563).
// NaN: every gate is written so that a NaN fails it on its own (the match is rejected AT that gate), where the reference's comparison
// would let it pass and create a point that is not a number.  UnprojectStereo of a depth that is not > 0 returns no point in the
// reference (whose next line then throws): here x3D is NaN and the match fails BEHIND_1.  x3D leaves triangulate_match with a NaN as the
// quiet NaN 0x7FC00000 (sim3::canon) so that host, device and Python store the same bytes.
#pragma once

#include "../../include/amos_frontend.h"
#include "amos_sim3_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace amos {
namespace newpt {

using pnp::fadd;
using pnp::fmul;
using pnp::fsub;
using sim3::canon;
using sim3::dot3;
using sim3::fdiv;

// cv::norm of a 3-vector, in double
FM_HD double norm3(float x, float y, float z)
{
    return fm::sqr(fm::add(fm::add(fm::mul((double)x, (double)x), fm::mul((double)y, (double)y)), fm::mul((double)z, (double)z)));
}
// Mat::dot of two 3-vectors, in double
FM_HD double mat_dot3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return fm::add(fm::add(fm::add(0.0, (double)fmul(a0, b0)), (double)fmul(a1, b1)), (double)fmul(a2, b2));
}
// one entry of R^T * x [+ t] as a gemm: column c of R against x
FM_HD float gemm3t(const float *R, int c, float x, float y, float z, float t)
{
    return (float)fm::add(dot3(R[c], R[3 + c], R[6 + c], x, y, z), (double)t);
}

// (float)(a * b) for row r of a and column c of b, both 3 x 3 row-major: one entry of a gemm
FM_HD float mm3(const float *a, const float *b, int r, int c) { return (float)dot3(a[3 * r], a[3 * r + 1], a[3 * r + 2], b[c], b[3 + c], b[6 + c]); }

// ComputeF12, the epipole and the baseline gate.  Returns false when the neighbour is skipped (|Ow2 - Ow1| < cam2.mb); g is written
// either way.
FM_HD bool pair_geometry(const amos_kf_camera &c1, const amos_kf_camera &c2, amos_kf_geometry *g)
{
    float R12[9], nR12[9], t12[3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {  // R1w * R2w.t()
            R12[3 * r + c] = (float)dot3(c1.Rcw[3 * r], c1.Rcw[3 * r + 1], c1.Rcw[3 * r + 2], c2.Rcw[3 * c], c2.Rcw[3 * c + 1], c2.Rcw[3 * c + 2]);
            nR12[3 * r + c] = -R12[3 * r + c];
        }
    for (int r = 0; r < 3; r++) t12[r] = sim3::gemm3(nR12, r, c2.tcw[0], c2.tcw[1], c2.tcw[2], c1.tcw[r]);
    const float t12x[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
    // K1^-T and K2^-1
    const float k1it[9] = {c1.invfx, 0.f, 0.f, 0.f, c1.invfy, 0.f, -fmul(c1.cx, c1.invfx), -fmul(c1.cy, c1.invfy), 1.f};
    const float k2i[9] = {c2.invfx, 0.f, -fmul(c2.cx, c2.invfx), 0.f, c2.invfy, -fmul(c2.cy, c2.invfy), 0.f, 0.f, 1.f};
    float m1[9], m2[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m1[3 * r + c] = mm3(k1it, t12x, r, c);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m2[3 * r + c] = mm3(m1, R12, r, c);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) g->f12[3 * r + c] = mm3(m2, k2i, r, c);
    // amos_adapt::epipole_in: C2 = R2w * Ow1 + t2w
    const float X = sim3::gemm3(c2.Rcw, 0, c1.Ow[0], c1.Ow[1], c1.Ow[2], c2.tcw[0]), Y = sim3::gemm3(c2.Rcw, 1, c1.Ow[0], c1.Ow[1], c1.Ow[2], c2.tcw[1]),
                Z = sim3::gemm3(c2.Rcw, 2, c1.Ow[0], c1.Ow[1], c1.Ow[2], c2.tcw[2]);
    const float invz = fdiv(1.0f, Z);
    g->ex = fadd(fmul(fmul(c2.fx, X), invz), c2.cx);
    g->ey = fadd(fmul(fmul(c2.fy, Y), invz), c2.cy);
    const float baseline = (float)norm3(fsub(c2.Ow[0], c1.Ow[0]), fsub(c2.Ow[1], c1.Ow[1]), fsub(c2.Ow[2], c1.Ow[2]));
    return !(baseline < c2.mb);
}

// cos(2 * atan2(mb / 2, d))
FM_HD float cos_stereo_parallax(float mb, float d)
{
    const float h = fdiv(mb, 2.0f);
    if (h == 0 && d == 0) return 1.0f;
    const double dd = fm::mul((double)d, (double)d), hh = fm::mul((double)h, (double)h);
    return (float)fm::dvd(fm::sub(dd, hh), fm::add(dd, hh));
}

// pnp::jacobi_sym(A, V, 4) with every index a constant: the same operations in the same order (tests/test_new_points_cpu.py holds the two
// together bit for bit), so that a lane keeps the two matrices in registers.
FM_HD void jacobi_sym4(double (&A)[16], double (&V)[16])
{
    using pnp::dvd;
    using pnp::fabs_;
    using pnp::sqr;
    constexpr int n = 4;
#pragma unroll
    for (int i = 0; i < 16; i++) V[i] = (i % 5) == 0 ? 1.0 : 0.0;
    for (int sweep = 0; sweep < pnp::kJacobiSweeps; sweep++) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < n; p++)
#pragma unroll
            for (int q = p + 1; q < n; q++) off = off + fabs_(A[p * n + q]);
        if (!(off > 0)) break;
#pragma unroll
        for (int p = 0; p + 1 < n; p++) {
#pragma unroll
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
#pragma unroll
                for (int k = 0; k < n; k++) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < n; k++) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                A[p * n + q] = 0.0;
                A[q * n + p] = 0.0;
#pragma unroll
                for (int k = 0; k < n; k++) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < n; k++) {  // sign: the largest |component| positive (the first on ties)
        double vm = V[k];
#pragma unroll
        for (int i = 1; i < n; i++) vm = fabs_(V[i * n + k]) > fabs_(vm) ? V[i * n + k] : vm;
        if (vm < 0)
#pragma unroll
            for (int i = 0; i < n; i++) V[i * n + k] = -V[i * n + k];
    }
}

// Row 3 of Vt of the 4 x 4 float32 matrix A (row-major), as floats
FM_HD void null_vector4(const float *A, float *v)
{
    double S[16], V[16];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double s = fm::mul((double)A[i], (double)A[j]);
#pragma unroll
            for (int k = 1; k < 4; k++) s = fm::add(s, fm::mul((double)A[4 * k + i], (double)A[4 * k + j]));
            S[4 * i + j] = s;
        }
    jacobi_sym4(S, V);
    double lam = S[0], v0 = V[0], v1 = V[4], v2 = V[8], v3 = V[12];  // pnp::eig_order(S, 4, false, .)[0]
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (S[5 * i] < lam) { lam = S[5 * i]; v0 = V[i]; v1 = V[4 + i]; v2 = V[8 + i]; v3 = V[12 + i]; }
    v[0] = (float)v0; v[1] = (float)v1; v[2] = (float)v2; v[3] = (float)v3;
}

// The rows of A (:486-489) from the two normalised points and the two poses
FM_HD void triangulation_rows(const amos_kf_camera &c1, const amos_kf_camera &c2, float xn1x, float xn1y, float xn2x, float xn2y, float *A)
{
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float t1r0 = c < 3 ? c1.Rcw[c] : c1.tcw[0], t1r1 = c < 3 ? c1.Rcw[3 + c] : c1.tcw[1], t1r2 = c < 3 ? c1.Rcw[6 + c] : c1.tcw[2];
        const float t2r0 = c < 3 ? c2.Rcw[c] : c2.tcw[0], t2r1 = c < 3 ? c2.Rcw[3 + c] : c2.tcw[1], t2r2 = c < 3 ? c2.Rcw[6 + c] : c2.tcw[2];
        A[c] = fsub(fmul(xn1x, t1r2), t1r0);
        A[4 + c] = fsub(fmul(xn1y, t1r2), t1r1);
        A[8 + c] = fsub(fmul(xn2x, t2r2), t2r0);
        A[12 + c] = fsub(fmul(xn2y, t2r2), t2r1);
    }
}

// x3D = vt.row(3)[0..2] / vt.row(3)[3] (:491-497); false: w == 0
FM_HD bool dehomogenise(const float *v, float *x3D)
{
    if (v[3] == 0) return false;
    const float inv = (float)fm::dvd(1.0, (double)v[3]);
    x3D[0] = fmul(v[0], inv); x3D[1] = fmul(v[1], inv); x3D[2] = fmul(v[2], inv);
    return true;
}

// KeyFrame::UnprojectStereo from the raw keypoint (u, v) and its depth; NaN when the depth is not > 0
FM_HD void unproject_stereo(const amos_kf_camera &c, float u, float v, float z, float *x3D)
{
    if (!(z > 0)) {
        x3D[0] = x3D[1] = x3D[2] = __builtin_nanf("");
        return;
    }
    const float x = fmul(fmul(fsub(u, c.cx), z), c.invfx), y = fmul(fmul(fsub(v, c.cy), z), c.invfy);
#pragma unroll
    for (int r = 0; r < 3; r++) x3D[r] = gemm3t(c.Rcw, r, x, y, z, c.Ow[r]);
}

// One keyframe's side of a match: the undistorted keypoint, the raw one, u_right and the depth
struct Feature {
    float x, y;        // mvKeysUn[i].pt
    int octave;        // mvKeysUn[i].octave
    float rawX, rawY;  // mvKeys[i].pt
    float uRight;      // mvuRight[i]: stereo when >= 0
    float depth;       // mvDepth[i]
};

// :508-575 for one keyframe, everything after x3D: the depth sign and the reprojection gate.  mbf is the CURRENT keyframe's for both
// sides (:563).  0: passed, 1: behind, 2: reprojection
FM_HD int view_gates(const amos_kf_camera &c, const Feature &f, bool stereo, float mbf, float sigma2, const float *x3D)
{
    const float z = (float)fm::add(mat_dot3(c.Rcw[6], c.Rcw[7], c.Rcw[8], x3D[0], x3D[1], x3D[2]), (double)c.tcw[2]);
    if (!(z > 0)) return 1;
    const float x = (float)fm::add(mat_dot3(c.Rcw[0], c.Rcw[1], c.Rcw[2], x3D[0], x3D[1], x3D[2]), (double)c.tcw[0]);
    const float y = (float)fm::add(mat_dot3(c.Rcw[3], c.Rcw[4], c.Rcw[5], x3D[0], x3D[1], x3D[2]), (double)c.tcw[1]);
    const float invz = (float)fm::dvd(1.0, (double)z);
    const float u = fadd(fmul(fmul(c.fx, x), invz), c.cx), v = fadd(fmul(fmul(c.fy, y), invz), c.cy);
    const float errX = fsub(u, f.x), errY = fsub(v, f.y);
    float e = fadd(fmul(errX, errX), fmul(errY, errY));
    double bound = 5.991;
    if (stereo) {
        const float uR = fsub(u, fmul(mbf, invz)), errR = fsub(uR, f.uRight);
        e = fadd(e, fmul(errR, errR));
        bound = 7.8;
    }
    return (double)e <= fm::mul(bound, (double)sigma2) ? 0 : 2;
}

// :577-597: the two distances and the scale-consistency test.  0: passed, else DISTANCE_ZERO or SCALE
FM_HD int scale_gate(const amos_kf_camera &c1, const amos_kf_camera &c2, int octave1, int octave2, const float *scale, const float *X)
{
    const float dist1 = (float)norm3(fsub(X[0], c1.Ow[0]), fsub(X[1], c1.Ow[1]), fsub(X[2], c1.Ow[2]));
    const float dist2 = (float)norm3(fsub(X[0], c2.Ow[0]), fsub(X[1], c2.Ow[1]), fsub(X[2], c2.Ow[2]));
    if (dist1 == 0 || dist2 == 0) return AMOS_NEW_POINT_DISTANCE_ZERO;
    const float ratioFactor = fmul(1.5f, c1.scale_factor);
    const float ratioDist = fdiv(dist2, dist1), ratioOctave = fdiv(scale[octave1], scale[octave2]);
    if (!(fmul(ratioDist, ratioFactor) >= ratioOctave && ratioDist <= fmul(ratioOctave, ratioFactor))) return AMOS_NEW_POINT_SCALE;
    return 0;
}

// :424-597 for one match.  scale / sigma2: the level tables [nLevels] (one set for both keyframes).  Returns an AMOS_NEW_POINT_* verdict;
// x3D is written for every verdict but OCTAVE and LOW_PARALLAX (there it is 0).
FM_HD int triangulate_match(const amos_kf_camera &c1, const amos_kf_camera &c2, const Feature &f1, const Feature &f2, const float *scale,
                            const float *sigma2, int nLevels, float *x3D)
{
    x3D[0] = x3D[1] = x3D[2] = 0.f;
    if ((unsigned)f1.octave >= (unsigned)nLevels || (unsigned)f2.octave >= (unsigned)nLevels) return AMOS_NEW_POINT_OCTAVE;
    const bool stereo1 = f1.uRight >= 0, stereo2 = f2.uRight >= 0;
    const float xn1x = fmul(fsub(f1.x, c1.cx), c1.invfx), xn1y = fmul(fsub(f1.y, c1.cy), c1.invfy);
    const float xn2x = fmul(fsub(f2.x, c2.cx), c2.invfx), xn2y = fmul(fsub(f2.y, c2.cy), c2.invfy);
    float ray1[3], ray2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        ray1[r] = gemm3t(c1.Rcw, r, xn1x, xn1y, 1.0f, 0.f);
        ray2[r] = gemm3t(c2.Rcw, r, xn2x, xn2y, 1.0f, 0.f);
    }
    const float cosRays = (float)fm::dvd(mat_dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]),
                                         fm::mul(norm3(ray1[0], ray1[1], ray1[2]), norm3(ray2[0], ray2[1], ray2[2])));
    float cosStereo1 = fadd(cosRays, 1.0f), cosStereo2 = cosStereo1;
    if (stereo1) cosStereo1 = cos_stereo_parallax(c1.mb, f1.depth);
    else if (stereo2) cosStereo2 = cos_stereo_parallax(c2.mb, f2.depth);
    const float cosStereo = cosStereo2 < cosStereo1 ? cosStereo2 : cosStereo1;  // std::min
    int verdict;
    if (cosRays < cosStereo && cosRays > 0 && (stereo1 || stereo2 || (double)cosRays < 0.9998)) {
        float A[16], v[4];
        triangulation_rows(c1, c2, xn1x, xn1y, xn2x, xn2y, A);
        null_vector4(A, v);
        x3D[0] = canon(v[0]); x3D[1] = canon(v[1]); x3D[2] = canon(v[2]);
        if (!dehomogenise(v, x3D)) return AMOS_NEW_POINT_W_ZERO;
        verdict = AMOS_NEW_POINT_TRIANGULATED;
    } else if (stereo1 && cosStereo1 < cosStereo2) {
        unproject_stereo(c1, f1.rawX, f1.rawY, f1.depth, x3D);
        verdict = AMOS_NEW_POINT_UNPROJECTED_1;
    } else if (stereo2 && cosStereo2 < cosStereo1) {
        unproject_stereo(c2, f2.rawX, f2.rawY, f2.depth, x3D);
        verdict = AMOS_NEW_POINT_UNPROJECTED_2;
    } else
        return AMOS_NEW_POINT_LOW_PARALLAX;
    const float X[3] = {x3D[0], x3D[1], x3D[2]};
    x3D[0] = canon(X[0]); x3D[1] = canon(X[1]); x3D[2] = canon(X[2]);
    const int g1 = view_gates(c1, f1, stereo1, c1.mbf, sigma2[f1.octave], X);
    if (g1 == 1) return AMOS_NEW_POINT_BEHIND_1;
    // (the reference tests both depths before either reprojection)
    const float z2 = (float)fm::add(mat_dot3(c2.Rcw[6], c2.Rcw[7], c2.Rcw[8], X[0], X[1], X[2]), (double)c2.tcw[2]);
    if (!(z2 > 0)) return AMOS_NEW_POINT_BEHIND_2;
    if (g1 == 2) return AMOS_NEW_POINT_REPROJECTION_1;
    if (view_gates(c2, f2, stereo2, c1.mbf, sigma2[f2.octave], X) != 0) return AMOS_NEW_POINT_REPROJECTION_2;
    const int sg = scale_gate(c1, c2, f1.octave, f2.octave, scale, X);
    if (sg != 0) return sg;
    return verdict;
}

}  // namespace newpt
}  // namespace amos
