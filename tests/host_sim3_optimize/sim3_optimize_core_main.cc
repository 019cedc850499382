// sim3_optimize_core_main.cc -- amos-slam_amd/csrc/amos_sim3_opt_core.h as a plain C++ program with its own main, for a build with
// -fsanitize=address,undefined (tests/test_sim3_optimization_cpu.py compiles and runs it).  Each argument is a case file:
//   int32 n1, n2, n_levels, 0;  amos_sim3_camera cams[2];  amos_sim3_opt_pair pair;  float inv_sigma2[n_levels];
//   amos_keypoint kps1[n1];  amos_sim3_point pts1[n1];  amos_keypoint kps2[n2];  amos_sim3_point pts2[n2];  int32 row[n1]
// and the output is the return value, the 256 bytes of the result record in hex, and the row on return.
#include <cstdio>
#include <cstring>
#include <vector>

#include "sim3_optimize_host.h"

template <class T>
static bool read_n(FILE *f, std::vector<T> &v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        FILE *f = std::fopen(argv[a], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        int32_t head[4];
        amos_sim3_camera cams[2];
        amos_sim3_opt_pair pair;
        bool ok = std::fread(head, sizeof(head), 1, f) == 1 && std::fread(cams, sizeof(cams), 1, f) == 1 && std::fread(&pair, sizeof(pair), 1, f) == 1 &&
                  head[0] >= 0 && head[0] <= 65536 && head[1] >= 0 && head[1] <= 65536 && head[2] >= 1 && head[2] <= AMOS_MAX_LEVELS;
        std::vector<float> sig(ok ? head[2] : 0);
        std::vector<amos_keypoint> k1(ok ? head[0] : 0), k2(ok ? head[1] : 0);
        std::vector<amos_sim3_point> p1(k1.size()), p2(k2.size());
        std::vector<int32_t> row(k1.size()), out(k1.size());
        ok = ok && read_n(f, sig) && read_n(f, k1) && read_n(f, p1) && read_n(f, k2) && read_n(f, p2) && read_n(f, row);
        std::fclose(f);
        if (!ok) { std::fprintf(stderr, "%s is not a case file\n", argv[a]); return 2; }
        amos_sim3_opt_result res;
        const int nIn = s3o_host::optimize(k1.data(), p1.data(), head[0], k2.data(), p2.data(), head[1], cams, row.data(), sig.data(), head[2], pair,
                                           out.data(), &res);
        std::printf("case %s\n%d\n", argv[a], nIn);
        const unsigned char *b = reinterpret_cast<const unsigned char *>(&res);
        for (size_t i = 0; i < sizeof(res); i++) std::printf("%02x", b[i]);
        std::printf("\n");
        for (size_t i = 0; i < out.size(); i++) std::printf("%d ", out[i]);
        std::printf("\n");
    }
    return 0;
}
