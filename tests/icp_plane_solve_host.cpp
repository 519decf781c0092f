// Test infrastructure only.  The solve fragment of point-to-plane ICP (csrc/gdm_icp_plane_solve.inc: scaling, Cholesky with the pivot
// test, back-substitution, Rodrigues, pose composition) compiled unchanged as host C++, so that tests/test_icp_plane_cpu.py can hold
// it to numpy and run it under the host sanitizers.  A program of its own; never loaded into python.
//   icp_plane_solve_host <in.bin>
// in.bin: raw f64 records of 42 values { A upper triangle (21), g (6), S, L2, pose [R | t] row-major (12), pivot_min }.
// stdout: one line per record, 32 values printed with %.17g:
//   degenerate (0 / 1), min_pivot, xi (6), R_new (9, fp64), t_new (3, fp64), the pose as the kernel stores it (12, rounded to fp32).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

static void solve(const double* rec, double* out)
{
    const double* ps = rec;
    const double* rt = rec + 29;
    const double pivot_min = rec[41];
#include "../geometric_aware_dense_matching_amd/csrc/gdm_icp_plane_solve.inc"
    out[0] = degenerate ? 1.0 : 0.0;
    out[1] = min_pivot;
    for (int i = 0; i < 6; ++i) out[2 + i] = xi[i];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            out[8 + 3 * i + j] = Rn[i][j];
            out[20 + 4 * i + j] = (double)(float)Rn[i][j];
        }
        out[17 + i] = tn[i];
        out[20 + 4 * i + 3] = (double)(float)tn[i];
    }
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s in.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const long count = ftell(f) / (42 * (long)sizeof(double));
    fseek(f, 0, SEEK_SET);
    double* rec = (double*)malloc((size_t)(count ? count : 1) * 42 * sizeof(double));
    if (!rec || fread(rec, 42 * sizeof(double), (size_t)count, f) != (size_t)count) { fprintf(stderr, "read failed\n"); return 2; }
    fclose(f);
    for (long i = 0; i < count; ++i) {
        double out[32];
        solve(rec + 42 * i, out);
        for (int k = 0; k < 32; ++k) printf(k ? " %.17g" : "%.17g", out[k]);
        printf("\n");
    }
    free(rec);
    return 0;
}
