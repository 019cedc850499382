// pose_core_main.cc -- amos_pose_core.h as plain C++ with its own main: reads edge lists and prints what optimize_host() makes of them as
// hex doubles, for tests/test_pose_optimization_cpu.py to compare with the Python restatement bit for bit.  No HIP, no Python.
//   g++ -O2 -std=c++17 -ffp-contract=off -o pose_core_main pose_core_main.cc        (add -fsanitize=address,undefined for a checked run)
//   pose_core_main CASE.bin ...     CASE.bin: int32 n; 17 floats (Rcw, tcw, fx, fy, cx, cy, mbf); n x {float u, v, ur, X, Y, Z, w; int32 feat}
#include <cstdio>
#include <vector>

#include "../../amos-slam_amd/csrc/amos_pose_core.h"

using namespace amos::po;

int main(int argc, char **argv)
{
    static_assert(sizeof(Edge) == 32 && sizeof(Out) == 272, "the records of amos_pose_core.h");
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        int32_t n = 0;
        float cam[17];
        if (fread(&n, sizeof(n), 1, f) != 1 || n < 0 || n > (1 << 20) || fread(cam, sizeof(float), 17, f) != 17) { fprintf(stderr, "bad header in %s\n", argv[a]); return 2; }
        std::vector<Edge> edges((size_t)n);
        if (n && fread(edges.data(), sizeof(Edge), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short file %s\n", argv[a]); return 2; }
        fclose(f);
        std::vector<unsigned char> outlier((size_t)n, 0);
        const Cam c{(double)cam[12], (double)cam[13], (double)cam[14], (double)cam[15], (double)cam[16]};
        Out o;
        const int ret = optimize_host(edges.data(), n, outlier.data(), cam, cam + 9, c, 0, o);
        printf("case %s\nreturn %d rounds %d\n", argv[a], ret, o.rounds);
        for (int i = 0; i < 12; i++) printf("Rt %a\n", o.Rt[i]);
        for (int i = 0; i < 12; i++) printf("Tcw %a\n", (double)o.Tcw[i]);
        for (int i = 0; i < 3; i++) printf("Ow %a\n", (double)o.Ow[i]);
        for (int r = 0; r < kRounds; r++) printf("round %d %d %a %a\n", o.iterations[r], o.trials[r], o.lambda[r], o.chi2[r]);
        printf("outlier ");
        for (int e = 0; e < n; e++) putchar(outlier[e] ? '1' : '0');
        printf("\n");
    }
    return 0;
}
