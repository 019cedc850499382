// amos_sim3_search_core.h -- the projection steps of ORBmatcher::SearchBySim3 (ORBmatcher.cc:1333-1335, :1377-1411 / :1466-1497), written
// once for host and device.  Included by amos_sim3_search.hip (k_sim3_search_12 / k_sim3_search_21); tests/host_sim3_search compiles it as
// plain C++.  tests/sim3_search_restatement.py is the same arithmetic in Python float32 / float64 and the tests hold both compilations to
// it with ==: every operation is rounded on its own, in source order (explicit _rn operations on the device, -ffp-contract=off on the
// host).  include/amos_frontend.h, "loop-closing Sim3 search", defines it.
#pragma once

#include "amos_sim3_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace amos {
namespace sim3 {

struct SearchHops {
    float sR12[9], t12[3];  // camera 2 -> camera 1
    float sR21[9], t21[3];  // camera 1 -> camera 2
};

// sR12 = s12 * R12;  sR21 = (1.0 / s12) * R12.t();  t21 = -sR21 * t12 (:1333-1335)
FM_HD void sim3_search_hops(const float *R12, const float *t12, float s12, SearchHops &h)
{
    const double s = (double)s12, inv = fm::dvd(1.0, s);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            h.sR12[3 * r + c] = (float)fm::mul(s, (double)R12[3 * r + c]);
            h.sR21[3 * r + c] = (float)fm::mul(inv, (double)R12[3 * c + r]);
        }
    for (int r = 0; r < 3; r++) {
        h.t12[r] = t12[r];
        h.t21[r] = (float)-dot3(h.sR21[3 * r], h.sR21[3 * r + 1], h.sR21[3 * r + 2], t12[0], t12[1], t12[2]);
    }
}

// why a source feature's point leaves one direction (the first three are decided before the projection, the last three behind it)
enum SearchExit {
    kSearchNoPoint = 1, kSearchMatched = 2, kSearchBehind = 3, kSearchImage = 4, kSearchNear = 5, kSearchFar = 6,
    kSearchEmpty = 7, kSearchNone = 8, kSearchAccepted = 9
};

struct SearchProjection {
    float u, v, dist;
    int level;
};

// One point of the source keyframe through its world pose (Rfw, tfw) and the hop into the other camera, projected with K = fx, fy, cx, cy
// (KF1's in both directions): 0 when its window is to be searched, or the exit.  scale: nLevels entries.
FM_HD int sim3_search_project(const float *Rfw, const float *tfw, const float *hopR, const float *hopT, const float *K, const float *P, float minD,
                              float maxD, const float *scale, int nLevels, float minX, float maxX, float minY, float maxY, SearchProjection &o)
{
    float a[3], c[3];
    to_camera(Rfw, tfw, P, a);
    to_camera(hopR, hopT, a, c);
    o.u = o.v = o.dist = 0.f;
    o.level = 0;
    if (c[2] < 0.0f) return kSearchBehind;
    float u, v;
    to_image(c[0], c[1], c[2], K[0], K[1], K[2], K[3], u, v);
    if (!(u >= minX && u < maxX && v >= minY && v < maxY)) return kSearchImage;  // KeyFrame::IsInImage: a NaN or an infinity fails it
    const float dist = (float)fm::sqr(dot3(c[0], c[1], c[2], c[0], c[1], c[2]));
    if (dist < fmul(0.8f, minD)) return kSearchNear;
    if (dist > fmul(1.2f, maxD)) return kSearchFar;
    const float ratio = fdiv(maxD, dist);
    int level = 0;
    for (int m = 0; m < nLevels; m++) level += ratio > scale[m] ? 1 : 0;
    o.u = u; o.v = v; o.dist = dist;
    o.level = level < nLevels - 1 ? level : nLevels - 1;
    return 0;
}

}  // namespace sim3
}  // namespace amos
