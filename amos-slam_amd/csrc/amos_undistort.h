// amos_undistort.h -- cv::undistortPoints for one point (OpenCV 4.5 cvUndistortPointsInternal with its default criteria: exactly 5
// fixed-point iterations, no epsilon test, double arithmetic, k = (k1, k2, p1, p2, k3), the remaining coefficients zero, R = I).
// undistort_normalised is the P = none form (normalised coordinates, doubles); undistort_point the P = K form as Frame::UndistortKeyPoints
// and Frame::ComputeImageBounds call it (Frame.cc:1052-1118, 1121-1170).  Shared by the keypoint kernel, the host-side image bounds and
// the image-point round trip of the PnP (amos_pnp_core.h).  Plain + - * / in the written order (the library builds with -ffp-contract=off).
#pragma once

#if defined(__HIPCC__)
#define AMOS_UD_HD __host__ __device__ inline
#else
#define AMOS_UD_HD inline
#endif

namespace amos {

AMOS_UD_HD void undistort_normalised(float u, float v, double fx, double fy, double cx, double cy, const double (&k)[5], double &xo, double &yo)
{
    const double ifx = 1. / fx, ify = 1. / fy;
    double x = ((double)u - cx) * ifx, y = ((double)v - cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = 1. / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        if (icdist < 0) {  // OpenCV gives up and returns the normalised input point
            x = ((double)u - cx) * ifx;
            y = ((double)v - cy) * ify;
            break;
        }
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    xo = x;
    yo = y;
}

AMOS_UD_HD void undistort_point(float u, float v, double fx, double fy, double cx, double cy, const double (&k)[5], float &xo, float &yo)
{
    double x, y;
    undistort_normalised(u, v, fx, fy, cx, cy, k, x, y);
    xo = (float)(fx * x + cx);  // RR = K * I; ww = 1
    yo = (float)(fy * y + cy);
}

}  // namespace amos
