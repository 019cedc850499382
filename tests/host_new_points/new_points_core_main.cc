// new_points_core_main.cc -- amos-slam_amd/csrc/amos_new_points_core.h (through new_points_host.h's loop) as a plain C++ program with its
// own main, for a build with -fsanitize=address,undefined (tests/test_new_points_cpu.py compiles and runs it).  Each argument is a case
// file: seven int32 (n_frames, n_pairs, capacity, n_levels, has_raw, has_right, has_enabled), then kps [frames][capacity], kps_raw (if
// has_raw), counts, u_right and depth (if has_right), cameras, pairs_1, pairs_2, match12, enabled (if has_enabled; one byte per pair),
// scale_factors, level_sigma2.  The output is, per pair, one line with the sixteen ints of its stats, one with its verdict row and one per
// new point (idx1, idx2, the bits of x3D, verdict).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "new_points_host.h"

template <class T>
static bool read_array(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        FILE *f = std::fopen(argv[a], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        int32_t h[7] = {0, 0, 0, 0, 0, 0, 0};
        bool ok = std::fread(h, sizeof(int32_t), 7, f) == 7 && h[0] >= 1 && h[0] <= 1024 && h[1] >= 1 && h[1] <= 64 && h[2] >= 1 && h[2] <= 65536 &&
                  h[3] >= 1 && h[3] <= AMOS_MAX_LEVELS;
        const size_t frames = ok ? h[0] : 0, pairs = ok ? h[1] : 0, cap = ok ? h[2] : 0, levels = ok ? h[3] : 0;
        std::vector<amos_keypoint> kps, raw;
        std::vector<int32_t> counts, p1, p2, match;
        std::vector<float> right, depth, scale, sigma2;
        std::vector<amos_kf_camera> cams;
        std::vector<uint8_t> enabled;
        ok = ok && read_array(f, kps, frames * cap) && (!h[4] || read_array(f, raw, frames * cap)) && read_array(f, counts, frames) &&
             (!h[5] || (read_array(f, right, frames * cap) && read_array(f, depth, frames * cap))) && read_array(f, cams, frames) &&
             read_array(f, p1, pairs) && read_array(f, p2, pairs) && read_array(f, match, pairs * cap) && (!h[6] || read_array(f, enabled, pairs)) &&
             read_array(f, scale, levels) && read_array(f, sigma2, levels);
        std::fclose(f);
        for (size_t k = 0; ok && k < pairs; k++) ok = p1[k] >= 0 && p1[k] < h[0] && p2[k] >= 0 && p2[k] < h[0];
        if (!ok) { std::fprintf(stderr, "%s is not a case file\n", argv[a]); return 2; }
        new_points_host::Input in;
        in.kps = kps.data(); in.kps_raw = h[4] ? raw.data() : nullptr; in.counts = counts.data();
        in.u_right = h[5] ? right.data() : nullptr; in.depth = h[5] ? depth.data() : nullptr;
        in.cameras = cams.data(); in.pairs_1 = p1.data(); in.pairs_2 = p2.data(); in.match12 = match.data();
        in.enabled = h[6] ? enabled.data() : nullptr; in.scale = scale.data(); in.sigma2 = sigma2.data();
        in.n_frames = h[0]; in.n_pairs = h[1]; in.capacity = h[2]; in.n_levels = h[3];
        std::vector<amos_new_point> out(pairs * cap);
        std::vector<int32_t> verdict(pairs * cap);
        std::vector<amos_new_points_stats> stats(pairs);
        new_points_host::run(in, out.data(), verdict.data(), stats.data());
        std::printf("case %s\n", argv[a]);
        for (size_t p = 0; p < pairs; p++) {
            const int32_t *s = &stats[p].n_matches;
            std::printf("stats");
            for (int k = 0; k < 16; k++) std::printf(" %d", s[k]);
            std::printf("\nverdict");
            for (size_t i = 0; i < cap; i++) std::printf(" %d", verdict[p * cap + i]);
            std::printf("\n");
            for (int e = 0; e < stats[p].n_new; e++) {
                const amos_new_point &r = out[p * cap + e];
                uint32_t b[3];
                std::memcpy(b, &r.x, 12);
                std::printf("new %d %d %u %u %u %d\n", r.idx1, r.idx2, b[0], b[1], b[2], r.verdict);
            }
        }
    }
    return 0;
}
