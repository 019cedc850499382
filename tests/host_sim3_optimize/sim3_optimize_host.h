// sim3_optimize_host.h -- amos-slam_amd/csrc/amos_sim3_opt_core.h as a complete single-threaded OptimizeSim3 on host arrays: the kernel's
// prologue (the correspondences of one pair) and so::optimize_host.  Shared by sim3_optimize_capi.cc and sim3_optimize_core_main.cc.
#pragma once

#include <cstring>
#include <vector>

#include "../../include/amos_frontend.h"
#include "../../amos-slam_amd/csrc/amos_sim3_core.h"
#include "../../amos-slam_amd/csrc/amos_sim3_opt_core.h"

namespace s3o_host
{

// cams [2]: keyframe 1's, keyframe 2's; row [n1] in, row_out [n1] out (they may be one array).  Returns nIn.
inline int optimize(const amos_keypoint *kps1, const amos_sim3_point *pts1, int n1, const amos_keypoint *kps2, const amos_sim3_point *pts2, int n2,
                    const amos_sim3_camera *cams, const int32_t *row, const float *inv_sigma2, int n_levels, const amos_sim3_opt_pair &pair,
                    int32_t *row_out, amos_sim3_opt_result *result)
{
    using namespace amos;
    static_assert(sizeof(so::Out) == sizeof(amos_sim3_opt_result), "so::Out is amos_sim3_opt_result");
    std::vector<so::Corr> corrs;
    int status = 0;
    for (int i = 0; i < n1; i++) {
        const int j = row[i];
        if (j < 0 || j >= n2) continue;
        if ((pts1[i].flags & AMOS_SIM3_POINT_SKIP) || (pts2[j].flags & AMOS_SIM3_POINT_SKIP)) continue;
        const int o1 = kps1[i].octave, o2 = kps2[j].octave;
        if (o1 < 0 || o1 >= n_levels || o2 < 0 || o2 >= n_levels) { status |= so::kStatusOctave; continue; }
        so::Corr e;
        sim3::to_camera(cams[0].Rcw, cams[0].tcw, pts1[i].pos, e.P1);
        sim3::to_camera(cams[1].Rcw, cams[1].tcw, pts2[j].pos, e.P2);
        e.o1[0] = kps1[i].x; e.o1[1] = kps1[i].y; e.o2[0] = kps2[j].x; e.o2[1] = kps2[j].y;
        e.w1 = inv_sigma2[o1]; e.w2 = inv_sigma2[o2];
        e.feat = i; e.j = j;
        corrs.push_back(e);
    }
    std::vector<unsigned char> bad(corrs.size() + 1, 0);
    so::Cams k;
    k.k1[0] = cams[0].fx; k.k1[1] = cams[0].fy; k.k1[2] = cams[0].cx; k.k1[3] = cams[0].cy;
    k.k2[0] = cams[1].fx; k.k2[1] = cams[1].fy; k.k2[2] = cams[1].cx; k.k2[3] = cams[1].cy;
    so::Out o;
    const int nIn = so::optimize_host(corrs.data(), (int)corrs.size(), bad.data(), pair.R12, pair.t12, pair.s12, pair.th2, pair.fix_scale, k,
                                      cams[1].Rcw, cams[1].tcw, status, o);
    for (int i = 0; i < n1; i++) row_out[i] = row[i];
    for (size_t c = 0; c < corrs.size(); c++)
        if (bad[c]) row_out[corrs[c].feat] = -1;
    std::memcpy(result, &o, sizeof(o));
    return nIn;
}

}  // namespace s3o_host
