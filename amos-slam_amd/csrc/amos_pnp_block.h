// amos_pnp_block.h -- EPnP over a point set by ONE WORK-GROUP, shared by k_pnp_ransac (amos_pnp.hip: solvePnPRansac's refit on the RANSAC
// inliers) and k_reloc_pnp_iterate (amos_reloc_pnp.hip: PnPsolver::Refine on the best inlier set).  The arithmetic is amos_pnp_core.h;
// pnp::epnp_serial is the same on one thread.  Every sum over the points is owned by one lane and runs in point order; the per-point alphas
// and image points go through a global scratch row (pnp::kEpnpScratch doubles per point); the 12 x 12 Jacobi's rotations are applied by a
// group of sixteen lanes (jacobi_sym_group: every element sees jacobi_sym's operations in jacobi_sym's order); the three beta sets (betas,
// Gauss-Newton) run on three lanes side by side; the other small dense steps (PCA, pseudo-inverse, R and t) on one lane.  Device-only,
// force-inlined; every thread of the work-group calls.
#pragma once
#include "amos_common.h"
#include "amos_pnp_core.h"

namespace amos {

constexpr int kJacobiGroup = 16;  // lanes of one wave that share a 12 x 12 Jacobi: a quarter wave, twelve of them at work

// what separates a group's LDS writes from its next reads: the lanes of a group sit in one wave and run in lockstep, and a wave's LDS
// accesses complete in order, so no hardware barrier is needed -- only the compiler must keep the accesses on their side of the line
__device__ __forceinline__ void group_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// pnp::jacobi_sym(A, V, n) by the kJacobiGroup consecutive lanes of a group (l = 0 .. 15, n <= 16; all of them call, together): the
// rotations, their order and every element's operations are jacobi_sym's -- the rotation's c and s are computed by every lane from the same
// three elements, then lane k applies the column update to row k, the row update to column k and V's update to its row k, which jacobi_sym
// does for k = 0 .. n - 1 in turn (the updates of different k touch different elements).  A and V lie in LDS.
template <int n>
__device__ __forceinline__ void jacobi_sym_group(double *Ap, double *Vp, int l)
{
    using pnp::dvd;
    using pnp::fabs_;
    using pnp::sqr;
    volatile double *A = Ap, *V = Vp;
    const bool on = l < n;
    if (on)
        for (int j = 0; j < n; j++) V[l * n + j] = l == j ? 1.0 : 0.0;
    group_sync();
    for (int sweep = 0; sweep < pnp::kJacobiSweeps; sweep++) {
        double off = 0.0;
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) off = off + fabs_(A[p * n + q]);
        if (!(off > 0)) break;  // 0, or not finite (the same value in every lane)
        for (int p = 0; p + 1 < n; p++) {
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                if (apq == 0) continue;
                const double app = A[p * n + p], aqq = A[q * n + q], g = 100.0 * fabs_(apq);
                group_sync();  // every lane has read the three elements
                if (fabs_(app) + g == fabs_(app) && fabs_(aqq) + g == fabs_(aqq)) {
                    if (l == 0) { A[p * n + q] = 0.0; A[q * n + p] = 0.0; }
                    group_sync();
                    continue;
                }
                const double theta = dvd(aqq - app, 2.0 * apq);
                double t = dvd(1.0, fabs_(theta) + sqr(theta * theta + 1.0));
                if (theta < 0) t = -t;
                const double c = dvd(1.0, sqr(t * t + 1.0)), s = t * c;
                if (on) {  // row l of the column update, row l of V
                    const double akp = A[l * n + p], akq = A[l * n + q];
                    A[l * n + p] = c * akp - s * akq;
                    A[l * n + q] = s * akp + c * akq;
                    const double vkp = V[l * n + p], vkq = V[l * n + q];
                    V[l * n + p] = c * vkp - s * vkq;
                    V[l * n + q] = s * vkp + c * vkq;
                }
                group_sync();
                if (on) {  // column l of the row update; A[p][q] and A[q][p] end as 0
                    const double apk = A[p * n + l], aqk = A[q * n + l];
                    A[p * n + l] = l == q ? 0.0 : c * apk - s * aqk;
                    A[q * n + l] = l == p ? 0.0 : s * apk + c * aqk;
                }
                group_sync();
            }
        }
    }
    group_sync();
    if (on) {  // sign of column l: the largest |component| positive (the first on ties)
        int im = 0;
        for (int i = 1; i < n; i++) im = fabs_(V[i * n + l]) > fabs_(V[im * n + l]) ? i : im;
        if (V[im * n + l] < 0)
            for (int i = 0; i < n; i++) V[i * n + l] = -V[i * n + l];
    }
    group_sync();
}

// the 12 x 12 step of pnp::epnp_serial when the kJacobiGroup lanes of a group call it together (all of them on the same points, MtM and E)
struct Jacobi12Group {
    int l;
    __device__ __forceinline__ void operator()(double *A, double *V) const
    {
        group_sync();  // the lanes' identical writes of MtM are done
        jacobi_sym_group<12>(A, V, l);
    }
};

struct EpnpShared {  // in LDS
    double M[144], E[144];  // 12 x 12 MtM and its eigenvectors
    double S[9], Cw[4][3], Ci[9];
    double Ccs[3][4][3], Sum[3][6], Abt[3][9], Rt[3][12], Rep[3];
    int Neg[3];
};

// pw_of(j, pw) gives the world point of point j in doubles, uv_of(j, u, v) its pixel in floats; what the caller wrote for them must be
// visible (a barrier behind it).  On return (behind a barrier) sh.Rt[w] and sh.Rep[w] hold R | t and the mean reprojection error of the
// three beta sets.
template <int kThreads, class Pixel, class PwOf, class UvOf>
__device__ __forceinline__ void block_epnp(EpnpShared &sh, int m, PwOf pw_of, UvOf uv_of, double fx, double fy, double cx, double cy, double *scr)
{
    constexpr int kScr = pnp::kEpnpScratch;
    const int t = threadIdx.x;
    const double dm = (double)m;
    if (t < 3) {  // control point 0: the centroid
        double acc = 0.0, pw[3];
        for (int j = 0; j < m; j++) { pw_of(j, pw); acc = acc + pw[t]; }
        sh.Cw[0][t] = fm::dvd(acc, dm);
    }
    __syncthreads();
    if (t < 6) {  // PW0^T PW0, upper triangle (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        const int r = t < 3 ? 0 : (t < 5 ? 1 : 2), c = t < 3 ? t : (t < 5 ? t - 2 : 2);
        double acc = 0.0, pw[3];
        for (int j = 0; j < m; j++) { pw_of(j, pw); acc = acc + (pw[r] - sh.Cw[0][r]) * (pw[c] - sh.Cw[0][c]); }
        sh.S[3 * r + c] = acc;
        sh.S[3 * c + r] = acc;
    }
    __syncthreads();
    if (t == 0) {
        double S[9], cw[4][3], ci[9];
        for (int k = 0; k < 9; k++) S[k] = sh.S[k];
        for (int k = 0; k < 3; k++) cw[0][k] = sh.Cw[0][k];
        pnp::control_points(S, m, cw, ci);
        for (int i = 1; i < 4; i++) for (int k = 0; k < 3; k++) sh.Cw[i][k] = cw[i][k];
        for (int k = 0; k < 9; k++) sh.Ci[k] = ci[k];
    }
    __syncthreads();
    for (int j = t; j < m; j += kThreads) {  // per point: alphas and the image point
        double pw[3], al[4], cw0[3] = {sh.Cw[0][0], sh.Cw[0][1], sh.Cw[0][2]}, ci[9];
        for (int k = 0; k < 9; k++) ci[k] = sh.Ci[k];
        pw_of(j, pw);
        pnp::alphas(ci, cw0, pw[0], pw[1], pw[2], al);
        float uf, vf;
        uv_of(j, uf, vf);
        double u, v;
        Pixel::at(uf, vf, fx, fy, cx, cy, u, v);
        double *o = scr + (size_t)j * kScr;
        o[0] = al[0]; o[1] = al[1]; o[2] = al[2]; o[3] = al[3]; o[4] = u; o[5] = v;
    }
    __syncthreads();
    if (t < 78) {  // MtM, one lane per upper-triangle entry (r, c), rows of M in order
        int r = 0, k = t;
        while (k >= 12 - r) { k -= 12 - r; r++; }
        const int c = r + k;
        double acc = 0.0;
        for (int j = 0; j < m; j++) {
            const double *o = scr + (size_t)j * kScr;
            double r1, r2, c1, c2;
            pnp::m_entries(o, o[4], o[5], fx, fy, cx, cy, r, r1, r2);
            pnp::m_entries(o, o[4], o[5], fx, fy, cx, cy, c, c1, c2);
            acc = acc + r1 * c1;
            acc = acc + r2 * c2;
        }
        sh.M[12 * r + c] = acc;
        sh.M[12 * c + r] = acc;
    }
    __syncthreads();
    if (t < kJacobiGroup) jacobi_sym_group<12>(sh.M, sh.E, t);  // the first lanes of wave 0
    __syncthreads();
    if (t < 3) {  // one lane per beta set (each builds the null-space vectors, L and rho for itself)
        int order[12];
        pnp::eig_order(sh.M, 12, false, order);
        double v[4][12], cw[4][3], L[60], rho[6];
        for (int i = 0; i < 4; i++) for (int k = 0; k < 12; k++) v[i][k] = sh.E[12 * k + order[i]];
        for (int i = 0; i < 4; i++) for (int k = 0; k < 3; k++) cw[i][k] = sh.Cw[i][k];
        pnp::l6x10_rho(v, cw, L, rho);
        const double *o0 = scr;  // the first point decides solve_for_sign
        const int w = t;
        double betas[4], ccs[4][3], pc[3];
        pnp::betas_for(L, rho, w + 1, betas);
        pnp::ccs_of(betas, v, ccs);
        pnp::pc_of(o0, ccs, false, pc);
        sh.Neg[w] = pc[2] < 0.0 ? 1 : 0;
        for (int i = 0; i < 4; i++) for (int k = 0; k < 3; k++) sh.Ccs[w][i][k] = ccs[i][k];
    }
    __syncthreads();
    if (t < 18) {  // sums of pc (3) and pw (3) per beta set
        const int w = t / 6, q = t % 6;
        double ccs[4][3];
        for (int i = 0; i < 4; i++) for (int k = 0; k < 3; k++) ccs[i][k] = sh.Ccs[w][i][k];
        double acc = 0.0;
        for (int j = 0; j < m; j++) {
            double x;
            if (q < 3) {
                double pc[3];
                pnp::pc_of(scr + (size_t)j * kScr, ccs, sh.Neg[w] != 0, pc);
                x = pc[q];
            } else {
                double pw[3];
                pw_of(j, pw);
                x = pw[q - 3];
            }
            acc = acc + x;
        }
        sh.Sum[w][q] = fm::dvd(acc, dm);
    }
    __syncthreads();
    if (t < 27) {  // ABt per beta set
        const int w = t / 9, e = t % 9, r = e / 3, c = e % 3;
        double ccs[4][3];
        for (int i = 0; i < 4; i++) for (int k = 0; k < 3; k++) ccs[i][k] = sh.Ccs[w][i][k];
        double acc = 0.0;
        for (int j = 0; j < m; j++) {
            double pc[3], pw[3];
            pnp::pc_of(scr + (size_t)j * kScr, ccs, sh.Neg[w] != 0, pc);
            pw_of(j, pw);
            acc = acc + (pc[r] - sh.Sum[w][r]) * (pw[c] - sh.Sum[w][3 + c]);
        }
        sh.Abt[w][e] = acc;
    }
    __syncthreads();
    if (t < 3) {  // R, t and the mean reprojection error per beta set
        double H[9], Rt[12];
        for (int k = 0; k < 9; k++) H[k] = sh.Abt[t][k];
        pnp::r_and_t(H, &sh.Sum[t][0], &sh.Sum[t][3], Rt);
        double acc = 0.0;
        for (int j = 0; j < m; j++) {
            const double *o = scr + (size_t)j * kScr;
            double pw[3];
            pw_of(j, pw);
            acc = acc + pnp::reproj_term(Rt, pw, o[4], o[5], fx, fy, cx, cy);
        }
        sh.Rep[t] = fm::dvd(acc, dm);
        for (int k = 0; k < 12; k++) sh.Rt[t][k] = Rt[k];
    }
    __syncthreads();
}

// the beta set with the smallest mean reprojection error (the first on ties)
__device__ __forceinline__ int epnp_pick(const EpnpShared &sh)
{
    int N = 0;
    if (sh.Rep[1] < sh.Rep[0]) N = 1;
    if (sh.Rep[2] < sh.Rep[N]) N = 2;
    return N;
}

}  // namespace amos
