// Robust pose fitting on the device, gfx950: batched RANSAC over the dense correspondences and point-to-point ICP refinement.
//
// RANSAC restates the reference's sequential loop (utils/pvn3d_eval_utils_kpls.py:79-124 best_fit_transform_with_RANSAC) for a
// whole batch with every hypothesis at once:
//   ransac_compact_kernel  one workgroup per crop: the selected correspondences (mask != 0) in point order, as six fp32 planes
//                          (A = matched model vertex, B = scene point) -- the reference's A = mdl[idx], B = cld[cls_msk]
//   ransac_hyp_kernel      one lane per (crop, hypothesis): h = 0 is the Kabsch fit of all selected pairs (the statistics of
//                          gdm_kabsch_stats_hip), h >= 1 the Kabsch fit of 4 pairs drawn by the counter-based hash of gdm.h
//   ransac_score_kernel    one wave per 4 hypotheses of a crop: integer inlier counts (ballot + popcount, no float atomics)
//   ransac_select_kernel   one workgroup per crop: the reference's selection rule on the counts, and the fp64 refit on the inliers
// ICP (pvn3d_eval_utils_kpls.py:126-212 icp) runs scene -> model: icp_transform_kernel maps the selected scene points into the model
// frame, the exact kNN (K = 1) finds the nearest vertex, icp_update_kernel refits the absolute pose from (model[nn], scene) in fp64
// and applies the reference's convergence rule per crop, freezing a crop on the device once it stops.
// icp_plane_update_kernel is the opt-in point-to-plane refiner (no counterpart in the reference): the same transform and search, then one
// Gauss-Newton step on n . (x - q) with optional normal gating and Huber weights, frozen and flagged when the crop is degenerate.
// The fit, the residual, the statistics, the reductions, the compaction and the two per-pair steps of ICP are gdm_pose_fit.h.
#include "gdm_pose_fit.h"

namespace {

constexpr int SCORE_HYP_PER_WAVE = 4;
constexpr int SCORE_HYP_PER_BLOCK = 4 * SCORE_HYP_PER_WAVE;        // 256 threads = 4 waves

// lowbias32 (include/gdm.h, GDM_RANSAC sampling)
__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// pts f32[B][6][N]: planes ax, ay, az, bx, by, bz of the selected pairs in point order; nsel i32[B] their number.
__global__ __launch_bounds__(256) void ransac_compact_kernel(const float* __restrict__ scene_xyz, long scene_bstride, int pt_stride,
                                                             int ch_stride, const float* __restrict__ model_xyz,
                                                             const int32_t* __restrict__ best_idx, const uint8_t* __restrict__ mask,
                                                             int N, int M, float* __restrict__ pts, int32_t* __restrict__ nsel)
{
    compact_pairs<false>(scene_xyz, scene_bstride, pt_stride, ch_stride, model_xyz, best_idx, mask, N, M, pts, nsel, nullptr, nullptr, nullptr);
}

// hyp f32[B][H][12]: hypothesis poses.  Crops with n < min_points get the identity (never scored).
__global__ __launch_bounds__(64) void ransac_hyp_kernel(const float* __restrict__ pts, const int32_t* __restrict__ nsel,
                                                        const double* __restrict__ stats, int N, int H, int min_points, uint32_t seed,
                                                        float* __restrict__ hyp)
{
    const int b = blockIdx.y;
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= H) return;
    float* o = hyp + ((long)b * H + h) * 12;
    const int n = nsel[b];
    if (n < min_points) {
        sentinel_pose(o);
        o[11] = 0.f;                                                // deliberate: [I | 0], not the sentinel, in these unscored rows
        return;
    }
    if (h == 0) {                                                   // pvn3d_eval_utils_kpls.py:95 curr_RT = best_fit_transform(A, B)
        kabsch_fit(stats + (long)b * 16, o);
        return;
    }
    const float* P = pts + (long)b * 6 * N;
    const uint32_t hb = mix32(mix32(seed ^ 0x9e3779b9u) ^ (uint32_t)b);
    double st[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) st[i] = 0.0;
    for (int s = 0; s < 4; ++s) {                                   // :115-118 np.random.randint(0, ptsnum, 4), with replacement
        const uint32_t r = mix32(hb ^ (uint32_t)(4 * h + s));
        const int k = (int)(((unsigned long long)r * (unsigned long long)n) >> 32);
        acc_pair(st, P[k], P[N + k], P[2 * N + k], P[3 * N + k], P[4 * N + k], P[5 * N + k]);
    }
    kabsch_fit(st, o);
}

// counts i32[B][H]: the inliers of every hypothesis, |R a + t - b| <= match_err (:104-106).
__global__ __launch_bounds__(256) void ransac_score_kernel(const float* __restrict__ pts, const int32_t* __restrict__ nsel,
                                                           const float* __restrict__ hyp, int N, int H, int min_points, float thr2,
                                                           int32_t* __restrict__ counts)
{
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h0 = blockIdx.x * SCORE_HYP_PER_BLOCK + wave * SCORE_HYP_PER_WAVE;
    if (h0 >= H) return;                                            // wave-uniform: no barrier below
    const int n = nsel[b];
    float rt[SCORE_HYP_PER_WAVE][12];
#pragma unroll
    for (int k = 0; k < SCORE_HYP_PER_WAVE; ++k) {
        const float* src = hyp + ((long)b * H + min(h0 + k, H - 1)) * 12;
#pragma unroll
        for (int e = 0; e < 12; ++e) rt[k][e] = src[e];
    }
    int c[SCORE_HYP_PER_WAVE] = {0, 0, 0, 0};
    if (n >= min_points) {
        const float* P = pts + (long)b * 6 * N;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const bool in = i < n;
            const int k = in ? i : 0;
            const float ax = P[k], ay = P[N + k], az = P[2 * N + k], bx = P[3 * N + k], by = P[4 * N + k], bz = P[5 * N + k];
#pragma unroll
            for (int q = 0; q < SCORE_HYP_PER_WAVE; ++q)
                c[q] += __popcll(__ballot(in && residual2(rt[q], ax, ay, az, bx, by, bz) <= thr2));
        }
    }
    if (lane == 0)
        for (int q = 0; q < SCORE_HYP_PER_WAVE; ++q)
            if (h0 + q < H) counts[(long)b * H + h0 + q] = c[q];
}

// The reference's sequential rule on the counts (:102-110): the FIRST h with c_h > fix_percent * n wins and is refit on its inliers;
// otherwise the largest c_h (lowest h on ties) wins without a refit.  No inlier at all -> the sentinel (the reference returns zeros).
__global__ __launch_bounds__(256) void ransac_select_kernel(const float* __restrict__ pts, const int32_t* __restrict__ nsel,
                                                            const float* __restrict__ hyp, const int32_t* __restrict__ counts, int N,
                                                            int H, int min_points, float thr2, double fix_percent,
                                                            float* __restrict__ RT, uint8_t* __restrict__ valid,
                                                            int32_t* __restrict__ winner)
{
    __shared__ int s_first[4], s_bc[4], s_bh[4];
    __shared__ double red[4][16];
    __shared__ float s_rt[12];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = nsel[b];
    float* o = RT + (long)b * 12;
    if (n < min_points) {                                           // evaluator.py:94-96
        if (threadIdx.x == 0) { sentinel_pose(o); valid[b] = 0; winner[b] = -1; }
        return;
    }
    const double lim = fix_percent * (double)n;
    int first = 0x7fffffff, bc = -1, bh = 0x7fffffff;
    for (int h = threadIdx.x; h < H; h += 256) {
        const int c = counts[(long)b * H + h];
        if ((double)c > lim && h < first) first = h;
        if (c > bc || (c == bc && h < bh)) { bc = c; bh = h; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        first = min(first, __shfl_xor(first, off, 64));
        const int oc = __shfl_xor(bc, off, 64), oh = __shfl_xor(bh, off, 64);
        if (oc > bc || (oc == bc && oh < bh)) { bc = oc; bh = oh; }
    }
    if (lane == 0) { s_first[wave] = first; s_bc[wave] = bc; s_bh[wave] = bh; }
    __syncthreads();
    first = s_first[0]; bc = s_bc[0]; bh = s_bh[0];
    for (int w = 1; w < 4; ++w) {
        first = min(first, s_first[w]);
        if (s_bc[w] > bc || (s_bc[w] == bc && s_bh[w] < bh)) { bc = s_bc[w]; bh = s_bh[w]; }
    }
    if (first == 0x7fffffff) {                                      // no early exit: the best hypothesis as it is
        if (threadIdx.x == 0) {
            if (bc <= 0) { sentinel_pose(o); valid[b] = 0; winner[b] = -1; }
            else {
                const float* src = hyp + ((long)b * H + bh) * 12;
                for (int e = 0; e < 12; ++e) o[e] = src[e];
                valid[b] = 1; winner[b] = bh;
            }
        }
        return;
    }
    if (threadIdx.x < 12) s_rt[threadIdx.x] = hyp[((long)b * H + first) * 12 + threadIdx.x];
    __syncthreads();
    float rt[12];
    for (int e = 0; e < 12; ++e) rt[e] = s_rt[e];
    refit_winner(pts + (long)b * 6 * N, N, n, rt, thr2, red, b, first, o, valid, winner);
}

// query f32[B,N,3] = R^T (b - t): the scene points in the model frame of the current pose.
__global__ __launch_bounds__(256) void icp_transform_kernel(const float* __restrict__ scene_xyz, long scene_bstride, int pt_stride,
                                                            int ch_stride, const float* __restrict__ RT, int N,
                                                            float* __restrict__ query)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* r = RT + (long)b * 12;
    const float* sp = scene_xyz + (long)b * scene_bstride + (long)i * pt_stride;
    const float dx = sp[0] - r[3], dy = sp[ch_stride] - r[7], dz = sp[2 * ch_stride] - r[11];
    float* q = query + ((long)b * N + i) * 3;
    q[0] = r[0] * dx + r[4] * dy + r[8] * dz;
    q[1] = r[1] * dx + r[5] * dy + r[9] * dz;
    q[2] = r[2] * dx + r[6] * dy + r[10] * dz;
}

// One ICP iteration of every active crop (:191-207): pairs (model[nn], scene) of the selected points (minus those farther than
// reject_dist when it is >= 0) -> fp64 statistics -> the absolute pose.  mean = mean pair distance before the update; the update is
// applied, then |err - mean| < tolerance stops the crop; err <- mean.  Fewer than min_points pairs: the crop stops unchanged.
__global__ __launch_bounds__(256) void icp_update_kernel(const float* __restrict__ scene_xyz, long scene_bstride, int pt_stride,
                                                         int ch_stride, const float* __restrict__ model_xyz, const int32_t* __restrict__ nn,
                                                         const float* __restrict__ d2, const uint8_t* __restrict__ mask, int N, int M,
                                                         float reject2, double tolerance, int min_points, float* __restrict__ RT,
                                                         uint8_t* __restrict__ active, int32_t* __restrict__ iters,
                                                         double* __restrict__ err)
{
    __shared__ double red[4][17];
    const int b = blockIdx.x;
    if (!active[b]) return;                                         // block-uniform
    const float* sp = scene_xyz + (long)b * scene_bstride;
    double acc[17];
#pragma unroll
    for (int i = 0; i < 17; ++i) acc[i] = 0.0;
    for_icp_pairs(mask, d2, nn, b, N, M, reject2, [&](int i, int j, float dd) {
        acc_pair(acc, model_xyz[3 * j], model_xyz[3 * j + 1], model_xyz[3 * j + 2], sp[(long)i * pt_stride],
                 sp[(long)i * pt_stride + ch_stride], sp[(long)i * pt_stride + 2 * ch_stride]);
        acc[16] += sqrt((double)dd);
    });
    double tot[17];
    block_sum<17>(acc, red, tot);
    if (threadIdx.x != 0) return;
    if (!(tot[0] >= (double)min_points)) { active[b] = 0; return; }
    kabsch_fit(tot, RT + (long)b * 12);
    iters[b] += 1;
    const double mean = tot[16] / tot[0];
    if (fabs(err[b] - mean) < tolerance) active[b] = 0;
    err[b] = mean;
}

// One point-to-plane Gauss-Newton iteration of every active crop (include/gdm.h gdm_icp_plane_update_hip): x = query (the scene
// point in the model frame), q / n = the nearest vertex and its unit normal.  Per thread the 30 fp64 sums of acc_plane_pair and the pair
// count, reduced in the fixed order of block_sum; thread 0 solves (gdm_icp_plane_solve.inc) and applies the stop rule of icp_update_kernel.
__global__ __launch_bounds__(256) void icp_plane_update_kernel(const float* __restrict__ scene_nrm, long scene_bstride, int pt_stride,
                                                               int ch_stride, const float* __restrict__ query,
                                                               const float* __restrict__ model_xyz, const float* __restrict__ model_nrm,
                                                               const int32_t* __restrict__ nn, const float* __restrict__ d2,
                                                               const uint8_t* __restrict__ mask, int N, int M, float reject2,
                                                               double normal_gate, double huber_delta, double tolerance, int min_points,
                                                               double pivot_min, float* __restrict__ RT, uint8_t* __restrict__ active,
                                                               int32_t* __restrict__ iters, double* __restrict__ err,
                                                               int32_t* __restrict__ status, int32_t* __restrict__ n_kept)
{
    __shared__ double red[4][30];
    __shared__ int cred[4];
    const int b = blockIdx.x;
    if (!active[b]) return;                                         // block-uniform
    double rt[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) rt[e] = (double)RT[(long)b * 12 + e];
    const float* sn = scene_nrm ? scene_nrm + (long)b * scene_bstride : nullptr;
    double acc[30];
#pragma unroll
    for (int i = 0; i < 30; ++i) acc[i] = 0.0;
    int cnt = 0;
    for_icp_pairs(mask, d2, nn, b, N, M, reject2, [&](int i, int j, float) {
        const double nx = (double)model_nrm[3 * j], ny = (double)model_nrm[3 * j + 1], nz = (double)model_nrm[3 * j + 2];
        if (sn) {                                                   // (R^T s) . n >= normal_gate keeps the pair
            const double sx = (double)sn[(long)i * pt_stride], sy = (double)sn[(long)i * pt_stride + ch_stride],
                         sz = (double)sn[(long)i * pt_stride + 2 * ch_stride];
            const double mx = rt[0] * sx + rt[4] * sy + rt[8] * sz;
            const double my = rt[1] * sx + rt[5] * sy + rt[9] * sz;
            const double mz = rt[2] * sx + rt[6] * sy + rt[10] * sz;
            if (!(mx * nx + my * ny + mz * nz >= normal_gate)) return;
        }
        const float* xq = query + ((long)b * N + i) * 3;
        acc_plane_pair(acc, (double)xq[0], (double)xq[1], (double)xq[2], nx, ny, nz, (double)model_xyz[3 * j],
                       (double)model_xyz[3 * j + 1], (double)model_xyz[3 * j + 2], huber_delta);
        cnt += 1;
    });
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = cnt;      // visible after block_sum's barrier
    double tot[30];
    block_sum<30>(acc, red, tot);
    if (threadIdx.x != 0) return;
    const int n_pairs = cred[0] + cred[1] + cred[2] + cred[3];
    if (n_kept) n_kept[b] = n_pairs;
    if (n_pairs < max(min_points, 6)) { active[b] = 0; status[b] = 2; return; }
    const double* ps = tot;
#include "gdm_icp_plane_solve.inc"
    if (degenerate) { active[b] = 0; status[b] = 3; return; }
    float* o = RT + (long)b * 12;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[4 * i + j] = (float)Rn[i][j];
        o[4 * i + 3] = (float)tn[i];
    }
    iters[b] += 1;
    const double mean = tot[29] / (double)n_pairs;
    if (fabs(err[b] - mean) < tolerance) { active[b] = 0; status[b] = 1; }
    err[b] = mean;
}

struct RansacWs {
    float* pts;
    float* hyp;
    int32_t* nsel;
    size_t bytes;
};

RansacWs ransac_ws(void* base, int B, int N, int H)
{
    RansacWs w;
    w.bytes = 0;
    w.pts = carve<float>(base, w.bytes, (size_t)B * 6 * N * sizeof(float), 256);
    w.hyp = carve<float>(base, w.bytes, (size_t)B * H * 12 * sizeof(float), 256);
    w.nsel = carve<int32_t>(base, w.bytes, (size_t)B * sizeof(int32_t), 256);
    return w;
}

} // namespace

extern "C" size_t gdm_ransac_workspace_bytes(int B, int N, int H)
{
    if (B < 1 || N < 1 || H < 1 || H > GDM_RANSAC_MAX_H) return 0;
    return ransac_ws(nullptr, B, N, H).bytes;
}

extern "C" int gdm_ransac_pose_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* model_xyz,
                                   const int32_t* best_idx, const uint8_t* mask, const double* stats, int B, int N, int M, int H,
                                   float match_err, double fix_percent, uint32_t seed, int min_points, void* workspace,
                                   size_t workspace_bytes, float* RT, uint8_t* valid, int32_t* counts, int32_t* winner, void* stream)
{
    int rc = pair_entry_check("gdm_ransac_pose_hip",
                              scene_xyz && model_xyz && best_idx && mask && stats && workspace && RT && valid && counts && winner, B, N, M,
                              true, scene_bstride, pt_stride, ch_stride, true);
    if (rc) return rc;
    GDM_CHECK_ARG(H >= 1 && H <= GDM_RANSAC_MAX_H, "gdm_ransac_pose_hip: H=%d not in [1,%d]", H, GDM_RANSAC_MAX_H);
    GDM_CHECK_ARG(match_err > 0.f && match_err < 1e18f, "gdm_ransac_pose_hip: match_err=%g must be > 0", (double)match_err);
    GDM_CHECK_ARG(fix_percent > 0.0 && fix_percent <= 1.0, "gdm_ransac_pose_hip: fix_percent=%g not in (0, 1]", fix_percent);
    GDM_CHECK_ARG(min_points >= 1, "gdm_ransac_pose_hip: min_points=%d must be >= 1", min_points);
    const RansacWs w = ransac_ws(workspace, B, N, H);
    GDM_CHECK_ARG(workspace_bytes >= w.bytes, "gdm_ransac_pose_hip: workspace of %zu bytes, %zu needed", workspace_bytes, w.bytes);
    GDM_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "gdm_ransac_pose_hip: workspace must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const float thr2 = match_err * match_err;
    hipLaunchKernelGGL(ransac_compact_kernel, dim3(B), dim3(256), 0, s, scene_xyz, scene_bstride, pt_stride, ch_stride, model_xyz,
                       best_idx, mask, N, M, w.pts, w.nsel);
    if ((rc = gdm_launch_status("ransac_compact_kernel"))) return rc;
    hipLaunchKernelGGL(ransac_hyp_kernel, dim3(gdm_cdiv(H, 64), B), dim3(64), 0, s, w.pts, w.nsel, stats, N, H, min_points, seed, w.hyp);
    if ((rc = gdm_launch_status("ransac_hyp_kernel"))) return rc;
    hipLaunchKernelGGL(ransac_score_kernel, dim3(gdm_cdiv(H, SCORE_HYP_PER_BLOCK), B), dim3(256), 0, s, w.pts, w.nsel, w.hyp, N, H,
                       min_points, thr2, counts);
    if ((rc = gdm_launch_status("ransac_score_kernel"))) return rc;
    hipLaunchKernelGGL(ransac_select_kernel, dim3(B), dim3(256), 0, s, w.pts, w.nsel, w.hyp, counts, N, H, min_points, thr2, fix_percent,
                       RT, valid, winner);
    return gdm_launch_status("ransac_select_kernel");
}

extern "C" int gdm_icp_transform_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* RT, int B,
                                     int N, float* query, void* stream)
{
    const int rc = pair_entry_check("gdm_icp_transform_hip", scene_xyz && RT && query, B, N, -1, true, scene_bstride, pt_stride, ch_stride, true);
    if (rc) return rc;
    hipLaunchKernelGGL(icp_transform_kernel, dim3(gdm_cdiv(N, 256), B), dim3(256), 0, (hipStream_t)stream, scene_xyz, scene_bstride,
                       pt_stride, ch_stride, RT, N, query);
    return gdm_launch_status("icp_transform_kernel");
}

extern "C" int gdm_icp_update_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* model_xyz,
                                  const int32_t* nn, const float* d2, const uint8_t* mask, int B, int N, int M, float reject_dist,
                                  double tolerance, int min_points, float* RT, uint8_t* active, int32_t* iters, double* err, void* stream)
{
    const int rc = pair_entry_check("gdm_icp_update_hip", scene_xyz && model_xyz && nn && d2 && mask && RT && active && iters && err, B, N, M,
                                    true, scene_bstride, pt_stride, ch_stride, false);
    if (rc) return rc;
    GDM_CHECK_ARG(tolerance >= 0.0, "gdm_icp_update_hip: tolerance=%g must be >= 0", tolerance);
    GDM_CHECK_ARG(min_points >= 1, "gdm_icp_update_hip: min_points=%d must be >= 1", min_points);
    const float reject2 = reject_dist >= 0.f ? reject_dist * reject_dist : -1.f;
    hipLaunchKernelGGL(icp_update_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, scene_xyz, scene_bstride, pt_stride, ch_stride,
                       model_xyz, nn, d2, mask, N, M, reject2, tolerance, min_points, RT, active, iters, err);
    return gdm_launch_status("icp_update_kernel");
}

extern "C" int gdm_icp_plane_update_hip(const float* scene_nrm, long scene_bstride, int pt_stride, int ch_stride, const float* query,
                                        const float* model_xyz, const float* model_nrm, const int32_t* nn, const float* d2,
                                        const uint8_t* mask, int B, int N, int M, float reject_dist, double normal_gate,
                                        double huber_delta, double tolerance, int min_points, double pivot_min, float* RT,
                                        uint8_t* active, int32_t* iters, double* err, int32_t* status, int32_t* n_pairs,
                                        void* stream)
{
    const int rc = pair_entry_check("gdm_icp_plane_update_hip",
                                    query && model_xyz && model_nrm && nn && d2 && mask && RT && active && iters && err && status, B, N, M,
                                    scene_nrm != nullptr, scene_bstride, pt_stride, ch_stride, false);
    if (rc) return rc;
    GDM_CHECK_ARG(!scene_nrm || (normal_gate >= -1.0 && normal_gate <= 1.0), "gdm_icp_plane_update_hip: normal_gate=%g not in [-1, 1]",
                  normal_gate);
    GDM_CHECK_ARG(tolerance >= 0.0, "gdm_icp_plane_update_hip: tolerance=%g must be >= 0", tolerance);
    GDM_CHECK_ARG(min_points >= 1, "gdm_icp_plane_update_hip: min_points=%d must be >= 1", min_points);
    GDM_CHECK_ARG(pivot_min > 0.0, "gdm_icp_plane_update_hip: pivot_min=%g must be > 0", pivot_min);
    GDM_CHECK_ARG(huber_delta == huber_delta, "gdm_icp_plane_update_hip: huber_delta is NaN");
    const float reject2 = reject_dist >= 0.f ? reject_dist * reject_dist : -1.f;
    hipLaunchKernelGGL(icp_plane_update_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, scene_nrm, scene_bstride, pt_stride,
                       ch_stride, query, model_xyz, model_nrm, nn, d2, mask, N, M, reject2, normal_gate, huber_delta, tolerance,
                       min_points, pivot_min, RT, active, iters, err, status, n_pairs);
    return gdm_launch_status("icp_plane_update_kernel");
}
