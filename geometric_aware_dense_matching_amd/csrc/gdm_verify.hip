// Pose verification against the observed depth, gfx950 (gdm_pose_verify_hip; include/gdm.h THE VERIFICATION RULE; DESIGN.md 6q;
// pose.verify_poses_numpy restates it bit for bit on evaluation.render_depth_numpy, which draws with pixel_rule.py).  Coverage and
// depth are the pixel rule of gdm_render_depth_hip, from its one copy in gdm_raster.h; the window clamp, the tile of a workgroup, the
// tile's z-buffer and the refusals shared with gdm_refine.hip are gdm_raster_tile.h.
//   pose_verify_kernel     one workgroup per (instance, candidate, tile of the instance's window).  A tile is kTile x kTile pixels
//                          counted from the window's clamped corner, and its z-buffer lives in LDS: 16 KiB of fp32 depth bits, so
//                          nine workgroups fit the 160 KiB of a CU beside each other.  draw_tile clears the tile and walks all F
//                          faces into it with LDS atomicMin; the kernel then classifies the tile's pixels against the observed
//                          depth and adds six integers per wave to counts.  Integer sums commute: the counts do not depend on
//                          arrival order.  No depth image reaches memory.
//   verify_select_kernel   one thread per instance: the fp64 score of every candidate in index order, the best eligible one.
// The grid covers every tile a window can have (cdiv(W, kTile) x cdiv(H, kTile)): the windows are device data the launcher does
// not read, and a workgroup whose tile lies outside its window returns before it touches LDS.  counts is cleared by a fill kernel,
// not a memset node (see gdm_bop.hip).  No allocation and no host read: the call captures in a hipGraph.
#include "gdm_common.h"
#include "gdm_raster_tile.h"

namespace {

constexpr int kThreads = 256;
constexpr unsigned kInfBits = 0x7f800000u;
constexpr int kCounters = 6;                                               // n_model, n_agree, n_front, n_behind, n_nodepth, q_agree

typedef unsigned long long u64;

__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <typename VT>
__global__ __launch_bounds__(kThreads) void pose_verify_kernel(const VT* __restrict__ verts, const int32_t* __restrict__ faces,
                                                               const double* __restrict__ RT, const double* __restrict__ Kmat,
                                                               int k_per_instance, const float* __restrict__ depth_obs,
                                                               int obs_per_instance, const int32_t* __restrict__ window, int C, int V,
                                                               int F, int H, int W, double near, float delta, float inv_delta_q,
                                                               int32_t* __restrict__ counts)
{
    __shared__ unsigned zt[kTile * kTile];
    const int i = blockIdx.z, c = blockIdx.y;
    TileBox t;
    if (!tile_of_block(clamped_window(window, i, H, W), blockIdx.x, W, t)) return;
    const int lane = threadIdx.x & 63;
    draw_tile<kThreads>(zt, t, verts, faces, V, F, RT + ((long)i * C + c) * 12, Kmat + (k_per_instance ? (long)i * 9 : 0), near, H, W);

    // THE VERIFICATION RULE, fp32
    const float* obs = depth_obs + (obs_per_instance ? (long)i * H * W : 0L);
    int n_agree = 0, n_front = 0, n_behind = 0, n_nodepth = 0, q = 0;
    const int tw = t.x1 - t.x0 + 1, th = t.y1 - t.y0 + 1;
    for (int k = threadIdx.x; k < tw * th; k += kThreads) {
        const int tx = k % tw, ty = k / tw;
        const unsigned bits = zt[ty * kTile + tx];
        if (bits >= kInfBits) continue;                                    // nothing drawn
        const float z_r = __uint_as_float(bits);
        const float z_o = obs[(long)(t.y0 + ty) * W + (t.x0 + tx)];
        if (!(z_o > 0.f)) { ++n_nodepth; continue; }
        const float d = z_o - z_r;
        const float a = fabsf(d);
        if (a <= delta) {
            ++n_agree;
            q += (int)floorf(a * inv_delta_q);
        } else if (d < -delta) {
            ++n_front;
        } else {
            ++n_behind;
        }
    }
    const int vals[kCounters] = {n_agree + n_front + n_behind + n_nodepth, n_agree, n_front, n_behind, n_nodepth, q};
    int32_t* out = counts + ((long)i * C + c) * kCounters;
#pragma unroll
    for (int j = 0; j < kCounters; ++j) {
        const int v = wave_sum_i32(vals[j]);
        if (lane == 0 && v) atomicAdd(&out[j], v);
    }
}

__global__ __launch_bounds__(kThreads) void verify_select_kernel(const int32_t* __restrict__ counts, const uint8_t* __restrict__ cand_valid,
                                                                 int n, int C, double front_weight, int min_px,
                                                                 double* __restrict__ score, int32_t* __restrict__ best)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    int win = -1;
    double top = 0.0;
    for (int c = 0; c < C; ++c) {
        const int32_t* k = counts + ((long)i * C + c) * kCounters;
        const double agree = (double)k[1], front = (double)k[2], behind = (double)k[3];
        const double den = (agree + behind) + front_weight * front;
        const double sc = (agree - (double)k[5] / 512.0) / fmax(1.0, den);
        score[(long)i * C + c] = sc;
        const bool eligible = (!cand_valid || cand_valid[(long)i * C + c] != 0) && k[0] >= min_px;
        if (eligible && (win < 0 || sc > top)) {
            win = c;
            top = sc;
        }
    }
    best[i] = win;
}

__global__ __launch_bounds__(kThreads) void zero_i32_kernel(int32_t* __restrict__ p, long count)
{
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < count; k += (long)gridDim.x * kThreads) p[k] = 0;
}

} // namespace

extern "C" int gdm_pose_verify_hip(const void* verts, int verts_f64, const int32_t* faces, const double* RT, const double* K,
                                   int k_per_instance, const float* depth_obs, int obs_per_instance, const int32_t* window,
                                   const uint8_t* cand_valid, int n, int C, int V, int F, int H, int W, double near, double delta,
                                   double front_weight, int min_px, int32_t* counts, double* score, int32_t* best, void* stream)
{
    GDM_CHECK_ARG(verts && faces && RT && K && depth_obs && counts && score && best, "gdm_pose_verify_hip: NULL pointer");
    // q_agree adds up to 256 per pixel (a rounding above it included: 257) into an int32
    int rc = tile_entry_check("gdm_pose_verify_hip", " would overflow q_agree", n, C, V, F, H, W, near, k_per_instance, obs_per_instance,
                              verts_f64);
    if (rc) return rc;
    GDM_CHECK_ARG(delta > 0.0 && delta <= 3.0e38, "gdm_pose_verify_hip: delta=%g must be positive and finite in fp32", delta);
    const float delta_f = (float)delta, inv_delta_q = (float)(256.0 / delta);
    GDM_CHECK_ARG(delta_f > 0.f && inv_delta_q > 0.f && inv_delta_q <= 3.0e38f,
                  "gdm_pose_verify_hip: delta=%g: delta or 256 / delta is not a positive finite fp32 number", delta);
    GDM_CHECK_ARG(front_weight >= 0.0, "gdm_pose_verify_hip: front_weight=%g must be >= 0", front_weight);
    GDM_CHECK_ARG(min_px >= 0, "gdm_pose_verify_hip: min_px=%d must be >= 0", min_px);
    const hipStream_t s = (hipStream_t)stream;
    const long words = (long)n * C * kCounters;
    const int fill_blocks = gdm_cdiv(words, kThreads) < 2048 ? gdm_cdiv(words, kThreads) : 2048;
    hipLaunchKernelGGL(zero_i32_kernel, dim3(fill_blocks), dim3(kThreads), 0, s, counts, words);
    rc = gdm_launch_status("zero_i32_kernel");
    if (rc) return rc;
    const dim3 grid((unsigned)(gdm_cdiv(W, kTile) * gdm_cdiv(H, kTile)), C, n);
    if (verts_f64)
        hipLaunchKernelGGL(pose_verify_kernel<double>, grid, dim3(kThreads), 0, s, (const double*)verts, faces, RT, K, k_per_instance,
                           depth_obs, obs_per_instance, window, C, V, F, H, W, near, delta_f, inv_delta_q, counts);
    else
        hipLaunchKernelGGL(pose_verify_kernel<float>, grid, dim3(kThreads), 0, s, (const float*)verts, faces, RT, K, k_per_instance,
                           depth_obs, obs_per_instance, window, C, V, F, H, W, near, delta_f, inv_delta_q, counts);
    rc = gdm_launch_status("pose_verify_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(verify_select_kernel, dim3(gdm_cdiv(n, kThreads)), dim3(kThreads), 0, s, counts, cand_valid, n, C, front_weight,
                       min_px, score, best);
    return gdm_launch_status("verify_select_kernel");
}
