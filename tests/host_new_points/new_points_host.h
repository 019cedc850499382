// new_points_host.h -- amos-slam_amd/csrc/amos_new_points_core.h as a complete single-threaded host loop over pairs and matches, on the
// arrays amos_match_new_points_batch_device takes (host copies of them) and with its outputs, the claim rule of include/amos_frontend.h
// included.  Test infrastructure: new_points_capi.cc binds it for Python, new_points_core_main.cc runs it as a plain program.
#ifndef NEW_POINTS_HOST_H
#define NEW_POINTS_HOST_H

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../amos-slam_amd/csrc/amos_new_points_core.h"

namespace new_points_host
{

struct Input {
    const amos_keypoint *kps, *kps_raw;  // [frames][capacity]; kps_raw may be NULL
    const int32_t *counts;               // [frames]
    const float *u_right, *depth;        // [frames][capacity] or NULL
    const amos_kf_camera *cameras;       // [frames]
    const int32_t *pairs_1, *pairs_2;    // [n_pairs]
    const int32_t *match12;              // [n_pairs][capacity]
    const uint8_t *enabled;              // [n_pairs] or NULL
    const float *scale, *sigma2;         // [n_levels]
    int32_t n_frames, n_pairs, capacity, n_levels;
};

inline amos::newpt::Feature feature_of(const Input &in, int slot, int idx)
{
    const size_t o = (size_t)slot * in.capacity + idx;
    const amos_keypoint *raw = in.kps_raw ? in.kps_raw : in.kps;
    amos::newpt::Feature f;
    f.x = in.kps[o].x; f.y = in.kps[o].y; f.octave = in.kps[o].octave;
    f.rawX = raw[o].x; f.rawY = raw[o].y;
    f.uRight = in.u_right ? in.u_right[o] : -1.0f;
    f.depth = f.uRight >= 0 ? in.depth[o] : -1.0f;
    return f;
}

// out_new [n_pairs][capacity] (records beyond n_new are left alone), out_verdict [n_pairs][capacity] or NULL, out_stats [n_pairs]
inline void run(const Input &in, amos_new_point *out_new, int32_t *out_verdict, amos_new_points_stats *out_stats)
{
    const int cap = in.capacity;
    std::vector<int32_t> verdict((size_t)in.n_pairs * cap, -1);  // before the claim rule; -2: a match12 entry outside keyframe 2
    std::vector<float> x3d((size_t)in.n_pairs * cap * 3, 0.f);
    auto runs = [&](int p) { return !in.enabled || in.enabled[p]; };
    for (int p = 0; p < in.n_pairs; p++) {
        if (!runs(p)) continue;
        const int s1 = in.pairs_1[p], s2 = in.pairs_2[p];
        const int n1 = std::min(std::max(in.counts[s1], 0), cap), n2 = std::min(std::max(in.counts[s2], 0), cap);
        for (int i = 0; i < n1; i++) {
            const int m = in.match12[(size_t)p * cap + i];
            if (m == -1) continue;
            if (m < 0 || m >= n2) { verdict[(size_t)p * cap + i] = -2; continue; }
            verdict[(size_t)p * cap + i] = amos::newpt::triangulate_match(in.cameras[s1], in.cameras[s2], feature_of(in, s1, i), feature_of(in, s2, m),
                                                                          in.scale, in.sigma2, in.n_levels, &x3d[((size_t)p * cap + i) * 3]);
        }
    }
    for (int p = 0; p < in.n_pairs; p++) {
        amos_new_points_stats st;
        std::memset(&st, 0, sizeof(st));
        for (int i = 0; i < cap; i++) {
            int v = runs(p) ? verdict[(size_t)p * cap + i] : -1;
            if (v == -2) { st.status |= AMOS_NEW_POINTS_BAD_MATCH; v = -1; }
            if (v >= 0 && v <= AMOS_NEW_POINT_UNPROJECTED_2)
                for (int q = 0; q < p; q++) {
                    const int vq = verdict[(size_t)q * cap + i];
                    if (in.pairs_1[q] == in.pairs_1[p] && runs(q) && vq >= 0 && vq <= AMOS_NEW_POINT_UNPROJECTED_2) { v = AMOS_NEW_POINT_CLAIMED; break; }
                }
            if (out_verdict) out_verdict[(size_t)p * cap + i] = v;
            if (v < 0) continue;
            st.n_verdict[v]++;
            st.n_matches++;
            if (v <= AMOS_NEW_POINT_UNPROJECTED_2) {
                amos_new_point &r = out_new[(size_t)p * cap + st.n_new++];
                r.idx1 = i; r.idx2 = in.match12[(size_t)p * cap + i];
                r.x = x3d[((size_t)p * cap + i) * 3]; r.y = x3d[((size_t)p * cap + i) * 3 + 1]; r.z = x3d[((size_t)p * cap + i) * 3 + 2];
                r.verdict = v;
            }
        }
        if (st.n_verdict[AMOS_NEW_POINT_OCTAVE]) st.status |= AMOS_NEW_POINTS_BAD_OCTAVE;
        out_stats[p] = st;
    }
}

}  // namespace new_points_host

#endif
