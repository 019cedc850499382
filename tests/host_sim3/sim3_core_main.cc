// sim3_core_main.cc -- amos_sim3_core.h as plain C++ with its own main: reads case files and prints what the host-compiled solver
// (sim3_host_solver.h) makes of them, floats as hex, for tests/test_sim3_cpu.py to compare with the Python restatement bit for bit.
// No HIP, no Python.
//   g++ -O2 -std=c++17 -ffp-contract=off -o sim3_core_main sim3_core_main.cc        (add -fsanitize=address,undefined for a checked run)
//   sim3_core_main CASE.bin ...
// CASE.bin: int32 n1, n2, n_levels, fix_scale, min_inliers, max_iterations, n_iterations, n_calls; double probability; uint64 seed;
//           2 x amos_sim3_camera; float level_sigma2[n_levels]; amos_keypoint kps1[n1]; amos_sim3_point points1[n1]; amos_keypoint kps2[n2];
//           amos_sim3_point points2[n2]; int32 match12[n1]
#include <cstdio>
#include <vector>

#include "sim3_host_solver.h"

template <class T>
static bool read_n(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        int32_t head[8];
        double probability = 0;
        uint64_t seed = 0;
        amos_sim3_camera cameras[2];
        if (fread(head, sizeof(int32_t), 8, f) != 8 || fread(&probability, sizeof(double), 1, f) != 1 || fread(&seed, sizeof(seed), 1, f) != 1 ||
            fread(cameras, sizeof(amos_sim3_camera), 2, f) != 2) { fprintf(stderr, "bad header in %s\n", argv[a]); return 2; }
        const int n1 = head[0], n2 = head[1], nLevels = head[2], nCalls = head[7];
        if (n1 < 0 || n1 > 65536 || n2 < 0 || n2 > 65536 || nLevels < 1 || nLevels > AMOS_MAX_LEVELS || nCalls < 0 || nCalls > 64) {
            fprintf(stderr, "bad sizes in %s\n", argv[a]);
            return 2;
        }
        std::vector<float> sigma2;
        std::vector<amos_keypoint> kps1, kps2;
        std::vector<amos_sim3_point> pts1, pts2;
        std::vector<int32_t> match12;
        if (!read_n(f, sigma2, (size_t)nLevels) || !read_n(f, kps1, (size_t)n1) || !read_n(f, pts1, (size_t)n1) || !read_n(f, kps2, (size_t)n2) ||
            !read_n(f, pts2, (size_t)n2) || !read_n(f, match12, (size_t)n1)) { fprintf(stderr, "short file %s\n", argv[a]); return 2; }
        fclose(f);
        amos_sim3_params par = {};
        par.probability = probability; par.min_inliers = head[4]; par.max_iterations = head[5]; par.n_iterations = head[6];
        par.fix_scale = head[3]; par.reset = 1; par.enabled = 1; par.seed = seed;
        sim3_host::Solver s(kps1.data(), pts1.data(), n1, kps2.data(), pts2.data(), n2, cameras, match12.data(), sigma2.data(), nLevels, par);
        printf("case %s\n", argv[a]);
        std::vector<uint8_t> inlier((size_t)n1 + 1, 0);
        std::vector<int32_t> matchOut((size_t)n1 + 1, -1);
        for (int call = 0; call < nCalls; call++) {
            amos_sim3_result r;
            s.iterate(par.n_iterations, &r, inlier.data(), matchOut.data());
            printf("call %d code %d has_sim3 %d no_more %d n_inliers %d N %d max_iterations %d iterations %d iterations_call %d best_inliers %d status %d\n",
                   call, r.code, r.has_sim3, r.no_more, r.n_inliers, r.n_correspondences, r.max_iterations, r.iterations, r.iterations_call,
                   r.best_inliers, r.status);
            printf("rng %llx\n", (unsigned long long)s.rng);
            printf("sim3");
            for (int k = 0; k < 9; k++) printf(" %a", (double)r.R12[k]);
            for (int k = 0; k < 3; k++) printf(" %a", (double)r.t12[k]);
            printf(" %a", (double)r.s12);
            for (int k = 0; k < 16; k++) printf(" %a", (double)r.T12[k]);
            printf("\ninlier ");
            for (int i = 0; i < n1; i++) putchar(r.code == 0 && inlier[i] ? '1' : '0');
            printf("\n");
        }
    }
    return 0;
}
