// loop_points_core_main.cc -- amos-slam_amd/csrc/amos_loop_points_core.h as a plain C++ program with its own main, for a build with
// -fsanitize=address,undefined (tests/test_loop_points_cpu.py compiles and runs it).  Each argument is a case file: int32 n, then n records
// of 16 floats (an Scw, row-major); the output is one line per record: index, then the bits of Rcw [9], tcw [3], Ow [3] and scw.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../amos-slam_amd/csrc/amos_loop_points_core.h"

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        FILE *f = std::fopen(argv[a], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        int32_t n = 0;
        bool ok = std::fread(&n, sizeof(n), 1, f) == 1 && n >= 0 && n <= (1 << 20);
        std::vector<float> scw(ok ? (size_t)n * 16 : 0);
        ok = ok && std::fread(scw.data(), sizeof(float), scw.size(), f) == scw.size();
        std::fclose(f);
        if (!ok) { std::fprintf(stderr, "%s is not a case file\n", argv[a]); return 2; }
        std::printf("case %s\n", argv[a]);
        for (int i = 0; i < n; i++) {
            amos::loop::Unscaled u;
            amos::loop::unscale(scw.data() + (size_t)16 * i, u);
            float out[16];
            std::memcpy(out, u.Rcw, sizeof(float) * 9);
            std::memcpy(out + 9, u.tcw, sizeof(float) * 3);
            std::memcpy(out + 12, u.Ow, sizeof(float) * 3);
            out[15] = u.scw;
            std::printf("%d", i);
            for (int k = 0; k < 16; k++) {
                uint32_t b;
                std::memcpy(&b, &out[k], 4);
                std::printf(" %u", b);
            }
            std::printf("\n");
        }
    }
    return 0;
}
