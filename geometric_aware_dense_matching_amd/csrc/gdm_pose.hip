// Batched, masked sufficient statistics for the least-squares pose fit (Kabsch), gfx950.
//
// Replaces the per-thread `.cpu().numpy()` + `best_fit_transform` of the reference's pose solve
//   /root/reference/evaluator.py:85-100 (selected scene points, matched model vertices)
//   /root/reference/utils/pvn3d_eval_utils_kpls.py:43-77 (centroids, H = AA^T BB, SVD)
// One workgroup per crop streams the crop's points once (HBM-bound: 12 B/point scene xyz + 4 B index +
// 1 B mask + a 12-B gathered model vertex) and emits 16 doubles: n, sum A (3), sum B (3), sum A B^T (9),
// A = model vertex matched to the point, B = scene point.  fp64 accumulation: H = sum A B^T - n cA cB^T cancels heavily.
// kabsch_solve_kernel turns the 16 statistics into [R|t] on the device, one lane per crop (no library SVD, no host
// synchronisation, so the whole step can be captured in a hipGraph).
#include "gdm_pose_fit.h"

namespace {

__global__ __launch_bounds__(256) void kabsch_stats_kernel(const float* __restrict__ scene_xyz, long scene_bstride, int pt_stride,
                                                           int ch_stride, const float* __restrict__ model_xyz,
                                                           const int32_t* __restrict__ best_idx, const uint8_t* __restrict__ mask,
                                                           int N, int M, double* __restrict__ out)
{
    __shared__ double red[4][16];
    const int b = blockIdx.x;
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    const float* sp = scene_xyz + (long)b * scene_bstride;
    for (int i = threadIdx.x; i < N; i += 256) {
        if (!mask[(long)b * N + i]) continue;
        int j = best_idx[(long)b * N + i];
        j = min(max(j, 0), M - 1);
        acc_pair(acc, model_xyz[3 * j], model_xyz[3 * j + 1], model_xyz[3 * j + 2], sp[(long)i * pt_stride],
                 sp[(long)i * pt_stride + ch_stride], sp[(long)i * pt_stride + 2 * ch_stride]);
    }
    wave_sums<16>(acc, red);
    if (threadIdx.x < 16) out[(long)b * 16 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// The fit itself (Horn's quaternion, fp64 Jacobi), one lane per crop.  The two solve kernels include the fragment gdm_kabsch_fit.inc
// themselves and do not call kabsch_fit, its wrapper: through the wrapper the same statements compile to other instructions.
__global__ __launch_bounds__(64) void kabsch_solve_kernel(const double* __restrict__ stats, int B, int min_points,
                                                          float* __restrict__ RT, uint8_t* __restrict__ valid)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* st = stats + (long)b * 16;
    const double n = st[0];
    float* o = RT + (long)b * 12;
    if (!(n >= (double)min_points)) {                                   // evaluator.py:94-96 sentinel pose
        sentinel_pose(o);
        valid[b] = 0;
        return;
    }
#include "gdm_kabsch_fit.inc"
    valid[b] = 1;
}

// Weighted statistics: [0] = sum w, sum w A, sum w B, sum w A B^T over the points with mask != 0 and a finite weight > 0 (others are
// skipped); count = the number of such points.  A = target[b, i] when `target` is given, else model_xyz[best_idx].
__global__ __launch_bounds__(256) void kabsch_stats_w_kernel(const float* __restrict__ scene_xyz, long scene_bstride, int pt_stride,
                                                             int ch_stride, const float* __restrict__ model_xyz,
                                                             const int32_t* __restrict__ best_idx, const float* __restrict__ target,
                                                             const float* __restrict__ weight, const uint8_t* __restrict__ mask,
                                                             int N, int M, double* __restrict__ out, int32_t* __restrict__ count)
{
    __shared__ double red[4][16];
    __shared__ int cred[4];
    const int b = blockIdx.x;
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    int cnt = 0;
    const float* sp = scene_xyz + (long)b * scene_bstride;
    for (int i = threadIdx.x; i < N; i += 256) {
        if (!mask[(long)b * N + i]) continue;
        const float wf = weight[(long)b * N + i];
        if (!weight_usable(wf)) continue;                               // NaN, inf, zero and negative weights are skipped
        double ax, ay, az;
        if (target) {
            const float* t = target + ((long)b * N + i) * 3;
            ax = t[0]; ay = t[1]; az = t[2];
        } else {
            int j = best_idx[(long)b * N + i];
            j = min(max(j, 0), M - 1);
            ax = model_xyz[3 * j]; ay = model_xyz[3 * j + 1]; az = model_xyz[3 * j + 2];
        }
        cnt += 1;
        acc_pair_w(acc, wf, ax, ay, az, sp[(long)i * pt_stride], sp[(long)i * pt_stride + ch_stride], sp[(long)i * pt_stride + 2 * ch_stride]);
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = cnt;          // visible after wave_sums' barrier
    wave_sums<16>(acc, red);
    if (threadIdx.x < 16) out[(long)b * 16 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (threadIdx.x == 16) count[b] = cred[0] + cred[1] + cred[2] + cred[3];
}

// The same fit with n = sum w (the fragment is scale-free in n); valid iff count >= min_points and sum w > 0.
__global__ __launch_bounds__(64) void kabsch_solve_w_kernel(const double* __restrict__ stats, const int32_t* __restrict__ count, int B,
                                                            int min_points, float* __restrict__ RT, uint8_t* __restrict__ valid)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* st = stats + (long)b * 16;
    const double n = st[0];
    float* o = RT + (long)b * 12;
    if (!(count[b] >= min_points) || !(n > 0.0)) {
        sentinel_pose(o);
        valid[b] = 0;
        return;
    }
#include "gdm_kabsch_fit.inc"
    valid[b] = 1;
}

} // namespace

extern "C" int gdm_kabsch_solve_hip(const double* stats, int B, int min_points, float* RT, uint8_t* valid, void* stream)
{
    GDM_CHECK_ARG(stats && RT && valid, "gdm_kabsch_solve_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1, "gdm_kabsch_solve_hip: bad shape");
    hipLaunchKernelGGL(kabsch_solve_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, stats, B, min_points, RT, valid);
    return gdm_launch_status("kabsch_solve_kernel");
}

extern "C" int gdm_kabsch_stats_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* model_xyz,
                                    const int32_t* best_idx, const uint8_t* mask, int B, int N, int M, double* out, void* stream)
{
    GDM_CHECK_ARG(scene_xyz && model_xyz && best_idx && mask && out, "gdm_kabsch_stats_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && N >= 1 && M >= 1, "gdm_kabsch_stats_hip: bad shape");
    hipLaunchKernelGGL(kabsch_stats_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, scene_xyz, scene_bstride, pt_stride, ch_stride,
                       model_xyz, best_idx, mask, N, M, out);
    return gdm_launch_status("kabsch_stats_kernel");
}

extern "C" int gdm_kabsch_stats_w_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* model_xyz,
                                      const int32_t* best_idx, const float* target, const float* weight, const uint8_t* mask, int B,
                                      int N, int M, double* out, int32_t* count, void* stream)
{
    GDM_CHECK_ARG(scene_xyz && weight && mask && out && count, "gdm_kabsch_stats_w_hip: NULL pointer");
    GDM_CHECK_ARG(target || (model_xyz && best_idx), "gdm_kabsch_stats_w_hip: NULL pointer (neither target nor model_xyz + best_idx)");
    GDM_CHECK_ARG(B >= 1 && N >= 1 && (target || M >= 1), "gdm_kabsch_stats_w_hip: bad shape");
    hipLaunchKernelGGL(kabsch_stats_w_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, scene_xyz, scene_bstride, pt_stride, ch_stride,
                       model_xyz, best_idx, target, weight, mask, N, M, out, count);
    return gdm_launch_status("kabsch_stats_w_kernel");
}

extern "C" int gdm_kabsch_solve_w_hip(const double* stats, const int32_t* count, int B, int min_points, float* RT, uint8_t* valid,
                                      void* stream)
{
    GDM_CHECK_ARG(stats && count && RT && valid, "gdm_kabsch_solve_w_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1, "gdm_kabsch_solve_w_hip: bad shape");
    hipLaunchKernelGGL(kabsch_solve_w_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, stats, count, B, min_points, RT, valid);
    return gdm_launch_status("kabsch_solve_w_kernel");
}
