// ORACLE -- test infrastructure only.  The pose-fit fragment of the product (csrc/gdm_kabsch_fit.inc, the Horn quaternion by fp64
// Jacobi that the Kabsch solve, RANSAC and ICP kernels include) compiled unchanged as host C++, so that its math can be checked
// against numpy's SVD on the CPU and run under the host sanitizers.  -DKABSCH_FIT_MAIN adds a file-to-file driver for that.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" void kabsch_fit_host(const double* st, float* o)
{
    const double n = st[0];
#include "../geometric_aware_dense_matching_amd/csrc/gdm_kabsch_fit.inc"
}

// stats f64[count][16] -> RT f32[count][12]
extern "C" void kabsch_fit_host_batch(const double* stats, long count, float* RT)
{
    for (long i = 0; i < count; ++i) kabsch_fit_host(stats + 16 * i, RT + 12 * i);
}

#ifdef KABSCH_FIT_MAIN
// kabsch_fit_host_san <stats.bin> <RT.bin>: raw f64[count][16] in, raw f32[count][12] out.
int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s stats.bin RT.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const long count = bytes / (16 * (long)sizeof(double));
    double* st = (double*)malloc((size_t)(count ? count : 1) * 16 * sizeof(double));
    float* rt = (float*)malloc((size_t)(count ? count : 1) * 12 * sizeof(float));
    if (!st || !rt || fread(st, 16 * sizeof(double), (size_t)count, f) != (size_t)count) { fprintf(stderr, "read failed\n"); return 2; }
    fclose(f);
    kabsch_fit_host_batch(st, count, rt);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(rt, 12 * sizeof(float), (size_t)count, f) != (size_t)count) { fprintf(stderr, "write failed\n"); return 2; }
    fclose(f);
    free(st);
    free(rt);
    return 0;
}
#endif
