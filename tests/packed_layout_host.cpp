// Test infrastructure only.  The packed activation layout (csrc/gdm_packed_act.h) compiled as plain host C++, so that
// tests/test_packed_layout_cpu.py can hold the header's offsets to the documented formula and run them under the host sanitizers.
// A program of its own; never loaded into python.
//   packed_layout_host B C H W
// stdout: "map <bytes(B)> <nchunk> <plane> <lo>", then one line "b g y x hi lo" per (image, 8-channel group g = c / 8, pixel): the byte
// offsets of the group's hi and lo granule, pixel(b, g / 16, y, x) + group(g % 16) and that + lo().
// The program marks every granule it prints in a buffer of bytes(B) bytes (an offset outside it ends the run with status 3, a
// granule marked twice with status 4), and checks that granule() and group(16 + q) say the same as pixel() + group(q) and lo() (status 5).
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../geometric_aware_dense_matching_amd/csrc/gdm_packed_act.h"

int main(int argc, char** argv)
{
    if (argc == 3) {                // packed_layout_host ok N: gdm_packed_out_ok(C, p) for C in [0, N) x p in {16-byte aligned, not}
        alignas(16) static unsigned char buf[32];
        for (int C = 0; C < atoi(argv[2]); ++C) printf("%d %d %d\n", C, (int)gdm_packed_out_ok(C, buf), (int)gdm_packed_out_ok(C, buf + 8));
        return 0;
    }
    if (argc != 5) { fprintf(stderr, "usage: %s B C H W | ok N\n", argv[0]); return 2; }
    const int B = atoi(argv[1]), C = atoi(argv[2]), H = atoi(argv[3]), W = atoi(argv[4]);
    if (B < 1 || C < 8 || C % 8 || H < 1 || W < 1) { fprintf(stderr, "bad shape\n"); return 2; }
    const gdm_packed_map pm{C, H, W};
    const size_t bytes = pm.bytes(B);
    printf("map %zu %d %ld %ld\n", bytes, pm.nchunk(), pm.plane(), pm.lo());
    std::vector<unsigned char> mark(bytes, 0);
    for (int b = 0; b < B; ++b)
        for (int g = 0; g < C / 8; ++g)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const int chunk = g / (GDM_PK_CHUNK / 8), q = g % (GDM_PK_CHUNK / 8);
                    const long base = pm.pixel(b, chunk, y, x);
                    const long off[2] = {base + pm.group(q), base + pm.group(q) + pm.lo()};
                    if (pm.granule(b, chunk, q, y, x) != off[0] || base + pm.group(GDM_PK_LO + q) != off[1]) return 5;
                    for (int k = 0; k < 2; ++k) {
                        if (off[k] < 0 || (size_t)off[k] + GDM_PK_GRANULE > bytes) return 3;
                        for (int i = 0; i < GDM_PK_GRANULE; ++i)
                            if (mark[off[k] + i]++) return 4;
                    }
                    printf("%d %d %d %d %ld %ld\n", b, g, y, x, off[0], off[1]);
                }
    return 0;
}
