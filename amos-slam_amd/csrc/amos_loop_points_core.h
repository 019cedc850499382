// amos_loop_points_core.h -- the decomposition of Scw at the head of ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
// (ORBmatcher.cc:397-403), written once for host and device.  Included by amos_loop_points.hip (k_loop_project and the host form's
// validation); tests/host_loop_points compiles it as plain C++.  tests/adaptor_prefilter.py (unscaled, centre) is the same arithmetic in
// Python float32 / float64 and the tests hold both compilations to it bit for bit: every operation is rounded on its own, in source order
// (explicit _rn operations on the device, -ffp-contract=off on the host).  include/amos_frontend.h, "loop-closing point search", defines it.
#pragma once

#include "amos_sim3_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace amos {
namespace loop {

struct Unscaled {
    float Rcw[9], tcw[3], Ow[3];
    float scw;
};

// Scw: 16 floats, row-major [s R | s t] over 0 0 0 1.
//   scw = (float) sqrt(row0 . row0), the squares summed in double left to right              (:399: sqrt(sRcw.row(0).dot(sRcw.row(0))))
//   Rcw = sRcw / scw, tcw = st / scw: one float32 product per element with (float)(1.0 / (double) scw)   (:400-401: Mat / float)
//   Ow  = -Rcw^T tcw: the products summed in double left to right, negated, one rounding                 (:402)
FM_HD void unscale(const float *Scw, Unscaled &o)
{
    const double n2 = fm::add(fm::add(fm::mul((double)Scw[0], (double)Scw[0]), fm::mul((double)Scw[1], (double)Scw[1])), fm::mul((double)Scw[2], (double)Scw[2]));
    o.scw = (float)fm::sqr(n2);
    const float inv = (float)fm::dvd(1.0, (double)o.scw);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) o.Rcw[3 * r + c] = sim3::fmul(Scw[4 * r + c], inv);
        o.tcw[r] = sim3::fmul(Scw[4 * r + 3], inv);
    }
    for (int c = 0; c < 3; c++)
        o.Ow[c] = (float)-fm::add(fm::add(fm::mul((double)o.Rcw[c], (double)o.tcw[0]), fm::mul((double)o.Rcw[3 + c], (double)o.tcw[1])),
                                  fm::mul((double)o.Rcw[6 + c], (double)o.tcw[2]));
}

}  // namespace loop
}  // namespace amos
