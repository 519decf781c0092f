// BOP pose errors on the device, gfx950: MSSD / MSPD (lib/pysixd/pose_error.py:131-179), a depth rasteriser and the VSD counts
// (pose_error.py:84-126 with lib/pysixd/visibility.py and misc.depth_im_to_dist_im_fast).  Everything that decides a result is fp64
// (vector fp64 is cheap on this part; the library is built with -ffp-contract=off), so evaluation.*_numpy restate the kernels.
//   mssd_mspd_max_kernel   one workgroup per (instance, tile of 512 model points): the estimate's points and projections are made once
//                          and stay in registers, the symmetric ground truths R_gt S_R, R_gt S_t + t_gt are formed 64 at a time in LDS
//                          and looped over the tile; the maximum over the tile goes wave shuffle -> LDS -> ONE integer atomicMax per
//                          (tile, symmetry) on the bit pattern of the non-negative double (ordered like the value; a NaN stays on top).
//                          The only temporary is err[2][n][S].
//   sym_min_kernel         one wave per (error, instance): the minimum over the symmetries, the first one on a tie.
//   raster_kernel          one thread per (instance, triangle) by the pixel rule of include/gdm.h.  gdm_raster.h holds its code and the
//                          drawing loop (draw_wave_triangles: a triangle whose clamped box holds more than kSmallBox pixels is drawn
//                          by its whole wave striding over the box; the instance index travels with it) for every rasteriser of the
//                          library; pixel_rule.py restates the rule for evaluation.render_depth_numpy.  Unsigned atomicMin on the
//                          fp32 bit pattern (shade): positive floats order like their bits and a minimum does not depend on arrival
//                          order.
//   vsd_counts_kernel      distance images, visibility masks and the pixel costs in one pass over the three depth images; counts are
//                          summed per thread, per wave, per workgroup, then one integer atomicAdd per workgroup and counter.
// No allocation and no host read in any entry point: they capture in a hipGraph.  Accumulators are cleared by fill_u32_kernel, not by
// hipMemsetAsync: replayed from a captured graph, the runtime's memset node left a 16-byte non-zero pattern in the VSD counters.
#include "gdm_common.h"
#include "gdm_raster.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPPT = 2;                                                    // model points a thread keeps in registers
constexpr int kTile = kThreads * kPPT;
constexpr int kSymChunk = 64;                                              // symmetric ground truths formed in LDS at a time
constexpr unsigned kInfBits = 0x7f800000u;

typedef unsigned long long u64;

__device__ __forceinline__ u64 dbits(double v) { return (u64)__double_as_longlong(v); }

__device__ __forceinline__ u64 wave_max_u64(u64 v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u64 o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void mssd_mspd_max_kernel(
    const double* __restrict__ RT_est, const double* __restrict__ RT_gt, const double* __restrict__ pts,
    const double* __restrict__ sym_R, const double* __restrict__ sym_t, const double* __restrict__ Kmat, int k_per_instance,
    int n, int M, int S, u64* __restrict__ err)
{
    __shared__ double gs[kSymChunk][12];                                   // rows of [R_gt S_R | R_gt S_t + t_gt]
    __shared__ u64 smax[2][kSymChunk];

    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63;
    const long tile0 = (long)blockIdx.x * kTile;
    double e[12], g[12], k[9];
#pragma unroll
    for (int i = 0; i < 12; ++i) { e[i] = RT_est[(long)b * 12 + i]; g[i] = RT_gt[(long)b * 12 + i]; }
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = Kmat[(k_per_instance ? (long)b * 9 : 0) + i];

    // the estimate's side, once per tile
    double mx[kPPT], my[kPPT], mz[kPPT], ex[kPPT], ey[kPPT], ez[kPPT], eu[kPPT], ev[kPPT];
    bool ok[kPPT];
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
        const long p = tile0 + (long)j * kThreads + t;
        ok[j] = p < M;
        mx[j] = ok[j] ? pts[p * 3] : 0.0;
        my[j] = ok[j] ? pts[p * 3 + 1] : 0.0;
        mz[j] = ok[j] ? pts[p * 3 + 2] : 0.0;
        ex[j] = ((e[0] * mx[j] + e[1] * my[j]) + e[2] * mz[j]) + e[3];
        ey[j] = ((e[4] * mx[j] + e[5] * my[j]) + e[6] * mz[j]) + e[7];
        ez[j] = ((e[8] * mx[j] + e[9] * my[j]) + e[10] * mz[j]) + e[11];
        const double h0 = (k[0] * ex[j] + k[1] * ey[j]) + k[2] * ez[j];
        const double h1 = (k[3] * ex[j] + k[4] * ey[j]) + k[5] * ez[j];
        const double h2 = (k[6] * ex[j] + k[7] * ey[j]) + k[8] * ez[j];
        eu[j] = h0 / h2;
        ev[j] = h1 / h2;
    }

    for (int s0 = 0; s0 < S; s0 += kSymChunk) {
        const int nc = S - s0 < kSymChunk ? S - s0 : kSymChunk;
        if (t < nc) {
            const double* sr = sym_R + (long)(s0 + t) * 9;
            const double* st = sym_t + (long)(s0 + t) * 3;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    gs[t][r * 4 + c] = (g[r * 4] * sr[c] + g[r * 4 + 1] * sr[3 + c]) + g[r * 4 + 2] * sr[6 + c];
                gs[t][r * 4 + 3] = ((g[r * 4] * st[0] + g[r * 4 + 1] * st[1]) + g[r * 4 + 2] * st[2]) + g[r * 4 + 3];
            }
        }
        if (t < 2 * kSymChunk) (&smax[0][0])[t] = 0;
        __syncthreads();
        for (int sl = 0; sl < nc; ++sl) {
            double q[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) q[i] = gs[sl][i];
            u64 m3 = 0, m2 = 0;
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                const double gx = ((q[0] * mx[j] + q[1] * my[j]) + q[2] * mz[j]) + q[3];
                const double gy = ((q[4] * mx[j] + q[5] * my[j]) + q[6] * mz[j]) + q[7];
                const double gz = ((q[8] * mx[j] + q[9] * my[j]) + q[10] * mz[j]) + q[11];
                const double dx = ex[j] - gx, dy = ey[j] - gy, dz = ez[j] - gz;
                const double d3 = sqrt((dx * dx + dy * dy) + dz * dz);
                const double h0 = (k[0] * gx + k[1] * gy) + k[2] * gz;
                const double h1 = (k[3] * gx + k[4] * gy) + k[5] * gz;
                const double h2 = (k[6] * gx + k[7] * gy) + k[8] * gz;
                const double du = eu[j] - h0 / h2, dv = ev[j] - h1 / h2;
                const double d2 = sqrt(du * du + dv * dv);
                if (ok[j]) {
                    const u64 b3 = dbits(d3), b2 = dbits(d2);
                    m3 = b3 > m3 ? b3 : m3;
                    m2 = b2 > m2 ? b2 : m2;
                }
            }
            m3 = wave_max_u64(m3);
            m2 = wave_max_u64(m2);
            if (lane == 0) {
                atomicMax(&smax[0][sl], m3);
                atomicMax(&smax[1][sl], m2);
            }
        }
        __syncthreads();
        if (t < nc) {
            atomicMax(&err[(long)b * S + s0 + t], smax[0][t]);
            atomicMax(&err[((long)n + b) * S + s0 + t], smax[1][t]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void sym_min_kernel(const double* __restrict__ err, int n, int S, double* __restrict__ mssd,
                                                     double* __restrict__ mspd, int32_t* __restrict__ best3, int32_t* __restrict__ best2)
{
    const int which = blockIdx.x / n, b = blockIdx.x % n, lane = threadIdx.x;
    const double* row = err + ((long)which * n + b) * S;
    double val = 0.0;
    int idx = INT32_MAX;                                                   // no symmetry seen yet
    for (int s = lane; s < S; s += 64) {
        const double v = row[s];
        if (idx == INT32_MAX || v < val) { val = v; idx = s; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double ov = __shfl_xor(val, d, 64);
        const int oi = __shfl_xor(idx, d, 64);
        if (oi != INT32_MAX && (idx == INT32_MAX || ov < val || (ov == val && oi < idx))) { val = ov; idx = oi; }
    }
    if (lane == 0) {
        (which ? mspd : mssd)[b] = val;
        (which ? best2 : best3)[b] = idx;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// rasteriser

template <typename VT>
__global__ __launch_bounds__(kThreads) void raster_kernel(const VT* __restrict__ verts, const int32_t* __restrict__ faces,
                                                          const double* __restrict__ RT, const double* __restrict__ Kmat,
                                                          int k_per_instance, int n, int V, int F, int H, int W, double near,
                                                          unsigned* __restrict__ zbuf)
{
    const long gid = (long)blockIdx.x * kThreads + threadIdx.x;
    TriSetup s = {};
    bool valid = gid < (long)n * F;
    int b = 0;
    if (valid) {
        b = (int)(gid / F);
        const int f = (int)(gid % F);
        bool swapped;
        valid = tri_setup(verts, V, faces[(long)f * 3], faces[(long)f * 3 + 1], faces[(long)f * 3 + 2], RT + (long)b * 12,
                          Kmat + (k_per_instance ? (long)b * 9 : 0), near, H, W, s, swapped);
    }
    draw_wave_triangles(s, valid, b, [=](int cb, int px, int py, unsigned bits) {
        shade(&zbuf[(long)cb * H * W + (long)py * W + px], bits, 0u);
    });
}

__global__ __launch_bounds__(kThreads) void fill_u32_kernel(unsigned* __restrict__ p, long count, unsigned v)
{
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < count; i += (long)gridDim.x * kThreads) p[i] = v;
}

__global__ __launch_bounds__(kThreads) void empty_to_zero_kernel(unsigned* __restrict__ p, long count)
{
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < count; i += (long)gridDim.x * kThreads)
        if (p[i] == kInfBits) p[i] = 0u;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// VSD

struct VsdTaus { double v[GDM_VSD_MAX_TAUS]; };

__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ float load_depth(const float* __restrict__ p, long i, int inf_is_empty)
{
    const float d = p[i];
    return inf_is_empty && __float_as_uint(d) == kInfBits ? 0.f : d;
}

__global__ __launch_bounds__(kThreads) void vsd_counts_kernel(const float* __restrict__ depth_est, const float* __restrict__ depth_gt,
                                                              const float* __restrict__ depth_test, long test_stride,
                                                              const double* __restrict__ Kmat, int k_per_instance, int H, int W,
                                                              float delta, VsdTaus taus, int T, double diameter, int inf_is_empty,
                                                              int32_t* __restrict__ counts, double* __restrict__ tl_sums)
{
    __shared__ int part_i[kThreads / 64][2 + GDM_VSD_MAX_TAUS];
    __shared__ double part_d[kThreads / 64][GDM_VSD_MAX_TAUS];

    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double* kk = Kmat + (k_per_instance ? (long)b * 9 : 0);
    const double fx = kk[0], fy = kk[4], cx = kk[2], cy = kk[5];
    const long P = (long)H * W;
    const float* de = depth_est + (long)b * P;
    const float* dg = depth_gt + (long)b * P;
    const float* dt = depth_test + (long)b * test_stride;

    int n_union = 0, n_inter = 0;
    int cost[GDM_VSD_MAX_TAUS];
    double tl[GDM_VSD_MAX_TAUS];
#pragma unroll
    for (int i = 0; i < GDM_VSD_MAX_TAUS; ++i) { cost[i] = 0; tl[i] = 0.0; }

    for (long i = (long)blockIdx.x * kThreads + t; i < P; i += (long)gridDim.x * kThreads) {
        const int row = (int)(i / W), col = (int)(i % W);
        const double pxn = ((double)col - cx) / fx, pyn = ((double)row - cy) / fy;
        const double ze = (double)load_depth(de, i, inf_is_empty), zg = (double)load_depth(dg, i, inf_is_empty), zt = (double)dt[i];
        const double a_e = pxn * ze, b_e = pyn * ze, a_g = pxn * zg, b_g = pyn * zg, a_t = pxn * zt, b_t = pyn * zt;
        const double dist_e = sqrt((a_e * a_e + b_e * b_e) + ze * ze);
        const double dist_g = sqrt((a_g * a_g + b_g * b_g) + zg * zg);
        const double dist_t = sqrt((a_t * a_t + b_t * b_t) + zt * zt);
        const bool no_test = dist_t == 0.0;
        const bool vis_g = ((float)dist_g - (float)dist_t <= delta || no_test) && dist_g > 0.0;
        const bool vis_e = (((float)dist_e - (float)dist_t <= delta || no_test) && dist_e > 0.0) || (vis_g && dist_e > 0.0);
        n_union += (vis_g || vis_e) ? 1 : 0;
        if (vis_g && vis_e) {
            ++n_inter;
            double d = fabs(dist_g - dist_e);
            if (diameter > 0.0) d /= diameter;
#pragma unroll
            for (int j = 0; j < GDM_VSD_MAX_TAUS; ++j) {
                if (j < T) {
                    cost[j] += d >= taus.v[j] ? 1 : 0;
                    if (tl_sums) {
                        const double c = d / taus.v[j];
                        tl[j] += c > 1.0 ? 1.0 : c;
                    }
                }
            }
        }
    }

    n_union = wave_sum_i32(n_union);
    n_inter = wave_sum_i32(n_inter);
    if (lane == 0) { part_i[wave][0] = n_union; part_i[wave][1] = n_inter; }
#pragma unroll
    for (int j = 0; j < GDM_VSD_MAX_TAUS; ++j) {
        if (j < T) {
            const int c = wave_sum_i32(cost[j]);
            if (lane == 0) part_i[wave][2 + j] = c;
            if (tl_sums) {
                const double sd = wave_sum_f64(tl[j]);
                if (lane == 0) part_d[wave][j] = sd;
            }
        }
    }
    __syncthreads();
    if (t < 2 + T) {
        int v = 0;
        for (int w = 0; w < kThreads / 64; ++w) v += part_i[w][t];
        if (v) atomicAdd(&counts[(long)b * (2 + T) + t], v);
    }
    if (tl_sums && t < T) {
        double v = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) v += part_d[w][t];
        if (v != 0.0) atomicAdd(&tl_sums[(long)b * T + t], v);
    }
}

// Clears `words` 32-bit words at p with one launch of fill_u32_kernel.
static int clear_words(void* p, long words, hipStream_t s)
{
    const int blocks = (int)(gdm_cdiv(words, kThreads) < 2048 ? gdm_cdiv(words, kThreads) : 2048);
    hipLaunchKernelGGL(fill_u32_kernel, dim3(blocks), dim3(kThreads), 0, s, (unsigned*)p, words, 0u);
    return gdm_launch_status("fill_u32_kernel");
}

} // namespace

extern "C" int gdm_mssd_mspd_hip(const double* RT_est, const double* RT_gt, const double* pts, const double* sym_R, const double* sym_t,
                                 const double* K, int k_per_instance, int n, int M, int S, double* err, double* mssd, double* mspd,
                                 int32_t* best_sym_mssd, int32_t* best_sym_mspd, void* stream)
{
    GDM_CHECK_ARG(RT_est && RT_gt && pts && sym_R && sym_t && K && err && mssd && mspd && best_sym_mssd && best_sym_mspd,
                  "gdm_mssd_mspd_hip: NULL pointer");
    GDM_CHECK_ARG(n >= 1 && n <= 32767, "gdm_mssd_mspd_hip: n=%d not in [1, 32767]", n);
    GDM_CHECK_ARG(M >= 1, "gdm_mssd_mspd_hip: M=%d must be positive", M);
    GDM_CHECK_ARG(S >= 1 && (long)n * S <= (1L << 30), "gdm_mssd_mspd_hip: S=%d not in [1, 2^30 / n]", S);
    GDM_CHECK_ARG(k_per_instance == 0 || k_per_instance == 1, "gdm_mssd_mspd_hip: k_per_instance=%d must be 0 or 1", k_per_instance);
    const hipStream_t s = (hipStream_t)stream;
    int rc = clear_words(err, (long)2 * n * S * 2, s);
    if (rc) return rc;
    hipLaunchKernelGGL(mssd_mspd_max_kernel, dim3(gdm_cdiv(M, kTile), n), dim3(kThreads), 0, s, RT_est, RT_gt, pts, sym_R, sym_t, K,
                       k_per_instance, n, M, S, (u64*)err);
    rc = gdm_launch_status("mssd_mspd_max_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(sym_min_kernel, dim3(2 * n), dim3(64), 0, s, err, n, S, mssd, mspd, best_sym_mssd, best_sym_mspd);
    return gdm_launch_status("sym_min_kernel");
}

extern "C" int gdm_render_depth_hip(const void* verts, int verts_f64, const int32_t* faces, const double* RT, const double* K,
                                    int k_per_instance, int n, int V, int F, int H, int W, double near, int keep_inf, float* depth,
                                    void* stream)
{
    GDM_CHECK_ARG(verts && faces && RT && K && depth, "gdm_render_depth_hip: NULL pointer");
    GDM_CHECK_ARG(n >= 1 && V >= 1 && F >= 1, "gdm_render_depth_hip: n=%d V=%d F=%d must be positive", n, V, F);
    GDM_CHECK_ARG(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "gdm_render_depth_hip: H=%d W=%d not in [1, 16384]", H, W);
    GDM_CHECK_ARG((long)n * F <= (1L << 30) && (long)n * H * W <= (1L << 40), "gdm_render_depth_hip: n=%d too large for F=%d H=%d W=%d",
                  n, F, H, W);
    GDM_CHECK_ARG(near >= 0.0, "gdm_render_depth_hip: near=%g must be >= 0", near);
    GDM_CHECK_ARG(k_per_instance == 0 || k_per_instance == 1, "gdm_render_depth_hip: k_per_instance=%d must be 0 or 1", k_per_instance);
    GDM_CHECK_ARG(verts_f64 == 0 || verts_f64 == 1, "gdm_render_depth_hip: verts_f64=%d must be 0 or 1", verts_f64);
    const hipStream_t s = (hipStream_t)stream;
    const long count = (long)n * H * W;
    const int fill_blocks = (int)(gdm_cdiv(count, kThreads) < 2048 ? gdm_cdiv(count, kThreads) : 2048);
    unsigned* zb = (unsigned*)depth;
    hipLaunchKernelGGL(fill_u32_kernel, dim3(fill_blocks), dim3(kThreads), 0, s, zb, count, kInfBits);
    int rc = gdm_launch_status("fill_u32_kernel");
    if (rc) return rc;
    const dim3 grid(gdm_cdiv((long)n * F, kThreads));
    if (verts_f64)
        hipLaunchKernelGGL(raster_kernel<double>, grid, dim3(kThreads), 0, s, (const double*)verts, faces, RT, K, k_per_instance, n, V,
                           F, H, W, near, zb);
    else
        hipLaunchKernelGGL(raster_kernel<float>, grid, dim3(kThreads), 0, s, (const float*)verts, faces, RT, K, k_per_instance, n, V, F,
                           H, W, near, zb);
    rc = gdm_launch_status("raster_kernel");
    if (rc || keep_inf) return rc;
    hipLaunchKernelGGL(empty_to_zero_kernel, dim3(fill_blocks), dim3(kThreads), 0, s, zb, count);
    return gdm_launch_status("empty_to_zero_kernel");
}

extern "C" int gdm_vsd_counts_hip(const float* depth_est, const float* depth_gt, const float* depth_test, int test_per_instance,
                                  const double* K, int k_per_instance, int n, int H, int W, double delta, const double* taus, int T,
                                  double diameter, int inf_is_empty, int32_t* counts, double* tl_sums, void* stream)
{
    GDM_CHECK_ARG(depth_est && depth_gt && depth_test && K && taus && counts, "gdm_vsd_counts_hip: NULL pointer");
    GDM_CHECK_ARG(n >= 1 && n <= 65535, "gdm_vsd_counts_hip: n=%d not in [1, 65535]", n);
    GDM_CHECK_ARG(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "gdm_vsd_counts_hip: H=%d W=%d not in [1, 16384]", H, W);
    GDM_CHECK_ARG(T >= 1 && T <= GDM_VSD_MAX_TAUS, "gdm_vsd_counts_hip: T=%d not in [1, %d]", T, GDM_VSD_MAX_TAUS);
    GDM_CHECK_ARG(diameter >= 0.0, "gdm_vsd_counts_hip: diameter=%g must be >= 0 (0: costs are not normalised)", diameter);
    GDM_CHECK_ARG(test_per_instance == 0 || test_per_instance == 1, "gdm_vsd_counts_hip: test_per_instance=%d must be 0 or 1",
                  test_per_instance);
    GDM_CHECK_ARG(k_per_instance == 0 || k_per_instance == 1, "gdm_vsd_counts_hip: k_per_instance=%d must be 0 or 1", k_per_instance);
    VsdTaus tv = {};
    for (int i = 0; i < T; ++i) {
        GDM_CHECK_ARG(taus[i] > 0.0, "gdm_vsd_counts_hip: taus[%d]=%g must be positive", i, taus[i]);
        tv.v[i] = taus[i];
    }
    const hipStream_t s = (hipStream_t)stream;
    int rc = clear_words(counts, (long)n * (2 + T), s);
    if (rc) return rc;
    if (tl_sums && (rc = clear_words(tl_sums, (long)n * T * 2, s)) != 0) return rc;
    const long P = (long)H * W;
    const int bx = (int)(gdm_cdiv(P, kThreads * 4) < 256 ? gdm_cdiv(P, kThreads * 4) : 256);
    hipLaunchKernelGGL(vsd_counts_kernel, dim3(bx, n), dim3(kThreads), 0, s, depth_est, depth_gt, depth_test,
                       test_per_instance ? P : 0L, K, k_per_instance, H, W, (float)delta, tv, T, diameter, inf_is_empty, counts, tl_sums);
    return gdm_launch_status("vsd_counts_kernel");
}
