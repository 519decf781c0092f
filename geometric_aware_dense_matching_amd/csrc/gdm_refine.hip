// Pose refinement against the observed depth by render-and-compare, gfx950 (gdm_pose_refine_depth_hip; include/gdm.h THE DEPTH
// REFINEMENT RULE; pose.refine_poses_depth_numpy restates it operation for operation, drawing with pixel_rule.py).
// Coverage and depth are the pixel rule of gdm_render_depth_hip from its one copy in gdm_raster.h; the window clamp, the tile of a
// workgroup and the tile's z-buffer are gdm_raster_tile.h, shared with gdm_verify.hip; the solve is gdm_icp_plane_solve.inc.
//   depth_refine_init_kernel    one thread per (instance, candidate): the pose copied to the output, status 0 or 4 (cand_valid == 0),
//                               iters, err and pairs cleared -- a kernel, not a memset node (see gdm_bop.hip).
//   depth_refine_accum_kernel   one workgroup per (instance, candidate, tile of the instance's window), built like pose_verify_kernel:
//                               draw_tile clears the LDS tile and walks all F faces into it 256 at a time.  The tile holds 64-bit
//                               keys (fp32 depth bits << 32 | face), 32 KiB, one LDS atomicMin per covered pixel: the nearest face,
//                               the lower index among equal depths, as gdm_render.hip keeps it in memory.  After the barrier every
//                               thread forms the fp64 terms of its pixels (acc_plane_pair, the step of icp_plane_update_kernel); the
//                               30 sums and the pair count are reduced in block_sum's order (gdm_pose_fit.h) and 32 threads store the row
//                               partial[i, c, tile, 0..31] (the sums, the count, a zero).  No floating-point atomic anywhere: the
//                               result does not depend on arrival order.
//   depth_refine_solve_kernel   one thread per (instance, candidate): clamps the window with the same clamped_window, adds the
//                               rows of exactly the tiles that window has in tile index order (a row no workgroup wrote is never
//                               read), applies the starved / degenerate / stop logic and writes pose, status, iters, err, pairs.
//                               The pose stays fp64.
// The entry enqueues the init kernel and `iters` pairs of the other two.  A candidate whose status is no longer 0 costs its
// workgroups one load: they return before touching LDS.  No allocation, no host read: the call captures in a hipGraph.
#include "gdm_pose_fit.h"
#include "gdm_raster_tile.h"

namespace {

constexpr int kThreads = 256;
constexpr unsigned kInfBits = 0x7f800000u;
constexpr int kSums = 30;                                                  // A (21), g (6), S, L2, E
constexpr int kRow = 32;                                                   // doubles per partial row: the sums, the pair count, a 0

typedef unsigned long long u64;

__global__ __launch_bounds__(kThreads) void depth_refine_init_kernel(const double* __restrict__ RT_in, const uint8_t* __restrict__ cand_valid,
                                                                     long count, double* __restrict__ RT, int32_t* __restrict__ status,
                                                                     int32_t* __restrict__ iters, double* __restrict__ err,
                                                                     int32_t* __restrict__ pairs)
{
    const long k = (long)blockIdx.x * kThreads + threadIdx.x;
    if (k >= count) return;
    for (int e = 0; e < 12; ++e) RT[k * 12 + e] = RT_in[k * 12 + e];
    status[k] = (cand_valid && cand_valid[k] == 0) ? 4 : 0;
    iters[k] = 0;
    err[k] = 0.0;
    pairs[k] = 0;
}

template <typename VT>
__global__ __launch_bounds__(kThreads) void depth_refine_accum_kernel(const VT* __restrict__ verts, const int32_t* __restrict__ faces,
                                                                      const double* __restrict__ RT, const double* __restrict__ Kmat,
                                                                      int k_per_instance, const float* __restrict__ depth_obs,
                                                                      int obs_per_instance, const int32_t* __restrict__ window,
                                                                      const int32_t* __restrict__ status, int C, int V, int F, int H,
                                                                      int W, double near, float reject, double huber, double min_cos,
                                                                      double* __restrict__ partial)
{
    __shared__ u64 zt[kTile * kTile];
    __shared__ double red[4][kSums];
    __shared__ int cred[4];
    const int i = blockIdx.z, c = blockIdx.y;
    if (status[(long)i * C + c] != 0) return;                              // frozen: block-uniform, before any LDS access
    TileBox t;
    if (!tile_of_block(clamped_window(window, i, H, W), blockIdx.x, W, t)) return;
    const int lane = threadIdx.x & 63;
    const double* rt = RT + ((long)i * C + c) * 12;
    const double* kk = Kmat + (k_per_instance ? (long)i * 9 : 0);
    draw_tile<kThreads>(zt, t, verts, faces, V, F, rt, kk, near, H, W);

    // THE DEPTH REFINEMENT RULE: the gate in fp32, the terms in fp64
    const float* obs = depth_obs + (obs_per_instance ? (long)i * H * W : 0L);
    const double fx = kk[0], fy = kk[4], cx = kk[2], cy = kk[5];
    double R[9], tr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        tr[a] = rt[4 * a + 3];
#pragma unroll
        for (int b = 0; b < 3; ++b) R[3 * a + b] = rt[4 * a + b];
    }
    double acc[kSums];
#pragma unroll
    for (int a = 0; a < kSums; ++a) acc[a] = 0.0;
    int cnt = 0;
    const int tw = t.x1 - t.x0 + 1, th = t.y1 - t.y0 + 1;
    for (int k = threadIdx.x; k < tw * th; k += kThreads) {
        const int tx = k % tw, ty = k / tw;
        const u64 key = zt[ty * kTile + tx];
        const unsigned bits = (unsigned)(key >> 32);
        if (bits >= kInfBits) continue;                                    // nothing drawn
        const float z_r = __uint_as_float(bits);
        const int u = t.x0 + tx, v = t.y0 + ty;
        const float z_o = obs[(long)v * W + u];
        if (!(z_o > 0.f)) continue;
        if (!(fabsf(z_o - z_r) <= reject)) continue;
        const long f = (long)(unsigned)(key & 0xffffffffu);               // a drawn face: its indices passed tri_setup's range test
        const long i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        const double ax = (double)verts[i0 * 3], ay = (double)verts[i0 * 3 + 1], az = (double)verts[i0 * 3 + 2];
        const double e1x = (double)verts[i1 * 3] - ax, e1y = (double)verts[i1 * 3 + 1] - ay, e1z = (double)verts[i1 * 3 + 2] - az;
        const double e2x = (double)verts[i2 * 3] - ax, e2y = (double)verts[i2 * 3 + 1] - ay, e2z = (double)verts[i2 * 3 + 2] - az;
        const double mx = e1y * e2z - e1z * e2y, my = e1z * e2x - e1x * e2z, mz = e1x * e2y - e1y * e2x;
        const double mm = (mx * mx + my * my) + mz * mz;
        if (!(mm > 0.0)) continue;                                         // a face without area in the object frame has no plane
        const double len = sqrt(mm);
        const double nx = mx / len, ny = my / len, nz = mz / len;
        const double zo = (double)z_o;
        const double ox = (zo * ((double)u - cx)) / fx, oy = (zo * ((double)v - cy)) / fy, oz = zo;
        if (min_cos > 0.0) {
            const double rnx = (R[0] * nx + R[1] * ny) + R[2] * nz;
            const double rny = (R[3] * nx + R[4] * ny) + R[5] * nz;
            const double rnz = (R[6] * nx + R[7] * ny) + R[8] * nz;
            const double dot = (rnx * ox + rny * oy) + rnz * oz;
            const double oo = (ox * ox + oy * oy) + oz * oz;
            if (fabs(dot) < min_cos * sqrt(oo)) continue;
        }
        const double dx = ox - tr[0], dy = oy - tr[1], dz = oz - tr[2];
        const double x = (R[0] * dx + R[3] * dy) + R[6] * dz;
        const double y = (R[1] * dx + R[4] * dy) + R[7] * dz;
        const double z = (R[2] * dx + R[5] * dy) + R[8] * dz;
        acc_plane_pair(acc, x, y, z, nx, ny, nz, ax, ay, az, huber);
        cnt += 1;
    }
    // fixed order: butterfly in each wave (wave_sums), then waves 0..3 as block_sum adds them
    cnt = wave_sum(cnt);
    if (lane == 0) cred[threadIdx.x >> 6] = cnt;                           // visible after wave_sums' barrier
    wave_sums<kSums>(acc, red);
    if (threadIdx.x < kRow) {
        const int tiles = ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
        double* row = partial + (((long)i * C + c) * tiles + blockIdx.x) * kRow;
        const int a = threadIdx.x;
        row[a] = a < kSums ? ((red[0][a] + red[1][a]) + red[2][a]) + red[3][a] : a == kSums ? (double)(((cred[0] + cred[1]) + cred[2]) + cred[3]) : 0.0;
    }
}

__global__ __launch_bounds__(kThreads) void depth_refine_solve_kernel(const double* __restrict__ partial, const int32_t* __restrict__ window,
                                                                      long count, int C, int H, int W, double tolerance, int min_px,
                                                                      double pivot_min, double* __restrict__ RT,
                                                                      int32_t* __restrict__ status, int32_t* __restrict__ iters,
                                                                      double* __restrict__ err, int32_t* __restrict__ pairs)
{
    const long k = (long)blockIdx.x * kThreads + threadIdx.x;
    if (k >= count) return;
    if (status[k] != 0) return;
    const int i = (int)(k / C);
    const int tiles_x = (W + kTile - 1) / kTile;
    const int tiles = tiles_x * ((H + kTile - 1) / kTile);
    const Win w = clamped_window(window, i, H, W);
    double tot[kRow];
    for (int a = 0; a < kRow; ++a) tot[a] = 0.0;
    if (w.x0 <= w.x1 && w.y0 <= w.y1) {
        const int nx = (w.x1 - w.x0) / kTile + 1, ny = (w.y1 - w.y0) / kTile + 1;    // the tiles whose workgroups stored a row
        for (int ty = 0; ty < ny; ++ty)
            for (int tx = 0; tx < nx; ++tx) {
                const double* row = partial + (k * tiles + (long)ty * tiles_x + tx) * kRow;
                for (int a = 0; a < kRow; ++a) tot[a] += row[a];
            }
    }
    const int n_pairs = (int)tot[kSums];
    pairs[k] = n_pairs;
    if (n_pairs < max(min_px, 6)) { status[k] = 2; return; }
    double* rt = RT + k * 12;
    const double* ps = tot;
#include "gdm_icp_plane_solve.inc"
    if (degenerate) { status[k] = 3; return; }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) rt[4 * a + b] = Rn[a][b];
        rt[4 * a + 3] = tn[a];
    }
    iters[k] += 1;
    const double mean = tot[29] / (double)n_pairs;
    if (fabs(err[k] - mean) < tolerance) status[k] = 1;
    err[k] = mean;
}

} // namespace

extern "C" size_t gdm_pose_refine_depth_workspace_bytes(int n, int C, int H, int W)
{
    // the shape limits alone: the other arguments stand in with values that pass
    if (tile_entry_check("gdm_pose_refine_depth_workspace_bytes", "", n, C, 1, 1, H, W, 0.0, 0, 0, 0)) return 0;
    return (size_t)gdm_cdiv(W, kTile) * gdm_cdiv(H, kTile) * n * C * kRow * sizeof(double);
}

extern "C" int gdm_pose_refine_depth_hip(const void* verts, int verts_f64, const int32_t* faces, const double* RT_in, const double* K,
                                         int k_per_instance, const float* depth_obs, int obs_per_instance, const int32_t* window,
                                         const uint8_t* cand_valid, int n, int C, int V, int F, int H, int W, double near, int iters,
                                         double reject, double huber, double min_cos, int min_px, double tolerance, double pivot_min,
                                         void* workspace, size_t workspace_bytes, double* RT, int32_t* status, int32_t* iters_out,
                                         double* err, int32_t* pairs, void* stream)
{
    const char* me = "gdm_pose_refine_depth_hip";
    GDM_CHECK_ARG(verts && faces && RT_in && K && depth_obs && workspace && RT && status && iters_out && err && pairs, "%s: NULL pointer", me);
    int rc = tile_entry_check(me, "", n, C, V, F, H, W, near, k_per_instance, obs_per_instance, verts_f64);
    if (rc) return rc;
    GDM_CHECK_ARG(iters >= 1 && iters <= 64, "%s: iters=%d not in [1, 64]", me, iters);
    GDM_CHECK_ARG(reject > 0.0 && reject <= 3.0e38 && (float)reject > 0.f, "%s: reject=%g must be positive and finite in fp32", me, reject);
    GDM_CHECK_ARG(huber >= 0.0, "%s: huber=%g must be >= 0 (0: off)", me, huber);
    GDM_CHECK_ARG(min_cos >= 0.0 && min_cos < 1.0, "%s: min_cos=%g not in [0, 1)", me, min_cos);
    GDM_CHECK_ARG(min_px >= 0, "%s: min_px=%d must be >= 0", me, min_px);
    GDM_CHECK_ARG(tolerance >= 0.0, "%s: tolerance=%g must be >= 0", me, tolerance);
    GDM_CHECK_ARG(pivot_min > 0.0, "%s: pivot_min=%g must be positive", me, pivot_min);
    const size_t need = gdm_pose_refine_depth_workspace_bytes(n, C, H, W);
    GDM_CHECK_ARG(workspace_bytes >= need, "%s: workspace_bytes=%zu < %zu (gdm_pose_refine_depth_workspace_bytes)", me, workspace_bytes, need);
    GDM_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", me);
    const hipStream_t s = (hipStream_t)stream;
    const long count = (long)n * C;
    const dim3 per_cand((unsigned)gdm_cdiv(count, kThreads));
    hipLaunchKernelGGL(depth_refine_init_kernel, per_cand, dim3(kThreads), 0, s, RT_in, cand_valid, count, RT, status, iters_out, err, pairs);
    rc = gdm_launch_status("depth_refine_init_kernel");
    if (rc) return rc;
    const dim3 grid((unsigned)(gdm_cdiv(W, kTile) * gdm_cdiv(H, kTile)), C, n);
    const float reject_f = (float)reject;
    double* partial = (double*)workspace;
    for (int it = 0; it < iters; ++it) {
        if (verts_f64)
            hipLaunchKernelGGL(depth_refine_accum_kernel<double>, grid, dim3(kThreads), 0, s, (const double*)verts, faces, RT, K,
                               k_per_instance, depth_obs, obs_per_instance, window, status, C, V, F, H, W, near, reject_f, huber, min_cos,
                               partial);
        else
            hipLaunchKernelGGL(depth_refine_accum_kernel<float>, grid, dim3(kThreads), 0, s, (const float*)verts, faces, RT, K,
                               k_per_instance, depth_obs, obs_per_instance, window, status, C, V, F, H, W, near, reject_f, huber, min_cos,
                               partial);
        rc = gdm_launch_status("depth_refine_accum_kernel");
        if (rc) return rc;
        hipLaunchKernelGGL(depth_refine_solve_kernel, per_cand, dim3(kThreads), 0, s, partial, window, count, C, H, W, tolerance, min_px,
                           pivot_min, RT, status, iters_out, err, pairs);
        rc = gdm_launch_status("depth_refine_solve_kernel");
        if (rc) return rc;
    }
    return 0;
}
