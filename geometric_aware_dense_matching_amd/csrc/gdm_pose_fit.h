// What the pose kernels share (gdm_pose.hip, gdm_pose_robust.hip, gdm_consensus.hip, gdm_refine.hip), each piece defined here once:
// the sentinel pose, the fit and the residual, the 16 pair statistics, the fixed-order block reduction, the compaction of the selected
// correspondences, the refit on a hypothesis' inliers, the ICP pair gate and the 30 point-to-plane sums; then, for the host, the
// argument checks and the workspace carving of the entries that consume pairs.  Scoring and refit agree on every inlier, the consensus
// fit equals Kabsch on clean matches and every reduction has one order BECAUSE they are these functions, not copies of them.
// Every kernel that reduces runs 256 threads = 4 waves.
#pragma once
#include "gdm_common.h"

namespace {

// evaluator.py:94-96: the pose of a crop that cannot be fitted, [I | (0, 0, -1000)].
__device__ __forceinline__ void sentinel_pose(float* o)
{
    o[0] = 1.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f;
    o[4] = 0.f; o[5] = 1.f; o[6] = 0.f; o[7] = 0.f;
    o[8] = 0.f; o[9] = 0.f; o[10] = 1.f; o[11] = -1000.f;
}

// [R | t] from the 16 statistics { n, sum A, sum B, sum A_i B_j }, n > 0 (a sum of weights serves: the fragment is scale-free in n).
__device__ __forceinline__ void kabsch_fit(const double* st, float* o)
{
    const double n = st[0];
#include "gdm_kabsch_fit.inc"
}

// Squared residual |R a + t - b|^2 in fp32, evaluated in one fixed order (scoring and refit must agree on every inlier).
__device__ __forceinline__ float residual2(const float* rt, float ax, float ay, float az, float bx, float by, float bz)
{
    const float ex = rt[0] * ax + rt[1] * ay + rt[2] * az + rt[3] - bx;
    const float ey = rt[4] * ax + rt[5] * ay + rt[6] * az + rt[7] - by;
    const float ez = rt[8] * ax + rt[9] * ay + rt[10] * az + rt[11] - bz;
    return ex * ex + ey * ey + ez * ez;
}

// One pair (A = model side, B = scene side) of weight w into the 16 statistics; w * a first, then the products with b.
__device__ __forceinline__ void acc_pair_w(double* acc, double w, double ax, double ay, double az, double bx, double by, double bz)
{
    const double wx = w * ax, wy = w * ay, wz = w * az;
    acc[0] += w;
    acc[1] += wx; acc[2] += wy; acc[3] += wz;
    acc[4] += w * bx; acc[5] += w * by; acc[6] += w * bz;
    acc[7] += wx * bx; acc[8] += wx * by; acc[9] += wx * bz;
    acc[10] += wy * bx; acc[11] += wy * by; acc[12] += wy * bz;
    acc[13] += wz * bx; acc[14] += wz * by; acc[15] += wz * bz;
}

// The weights a weighted fit takes: finite and > 0.  NaN, infinite, zero and negative weights are skipped, here and in the backward of
// the pose loss, which must skip exactly the points the statistics skipped.
__device__ __forceinline__ bool weight_usable(float wf) { return (wf > 0.f) && (wf <= 3.402823466e38f); }

// The unweighted pair: 1.0 * a is a exactly and nothing is contracted (-ffp-contract=off), so this is the plain sum.
__device__ __forceinline__ void acc_pair(double* acc, double ax, double ay, double az, double bx, double by, double bz)
{
    acc_pair_w(acc, 1.0, ax, ay, az, bx, by, bz);
}

__device__ __forceinline__ int wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// NA per-thread accumulators summed over each wave of a 256-thread block by one butterfly (o = 32 ... 1) and left in red[wave][];
// ends with the barrier that makes red, and whatever else was stored to LDS before the call, visible to the block.
template <int NA>
__device__ __forceinline__ void wave_sums(double* acc, double (*red)[NA])
{
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        double v = acc[i];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        acc[i] = v;
    }
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < NA; ++i) red[threadIdx.x >> 6][i] = acc[i];
    __syncthreads();
}

// wave_sums, then waves 0..3 left to right: every thread gets the totals in tot[].
template <int NA>
__device__ __forceinline__ void block_sum(double* acc, double (*red)[NA], double* tot)
{
    wave_sums<NA>(acc, red);
    for (int i = 0; i < NA; ++i) tot[i] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
}

// One workgroup per crop: the selected correspondences (mask != 0) in point order as six fp32 planes pts f32[B][6][N] (ax, ay, az =
// the matched model vertex, bx, by, bz = the scene point) and their number nsel i32[B].  kIndexed: also sel i32[B][N], the point index
// of compacted k (k < nsel), and score / degree i32[B][N] set to -1 for every point.
template <bool kIndexed>
__device__ __forceinline__ void compact_pairs(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride,
                                              const float* model_xyz, const int32_t* best_idx, const uint8_t* mask, int N, int M,
                                              float* pts, int32_t* nsel, int32_t* sel, int32_t* score, int32_t* degree)
{
    __shared__ int wtot[4];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* sp = scene_xyz + (long)b * scene_bstride;
    float* P = pts + (long)b * 6 * N;
    int run = 0;
    for (int c0 = 0; c0 < N; c0 += 256) {
        const int i = c0 + threadIdx.x;
        const bool on = i < N && mask[(long)b * N + i];
        const unsigned long long bal = __ballot(on);
        const int below = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        int off = run;
        for (int w = 0; w < wave; ++w) off += wtot[w];
        if (kIndexed && i < N) { score[(long)b * N + i] = -1; degree[(long)b * N + i] = -1; }
        if (on) {
            int j = best_idx[(long)b * N + i];
            j = min(max(j, 0), M - 1);
            const int k = off + below;
            P[k] = model_xyz[3 * j];
            P[N + k] = model_xyz[3 * j + 1];
            P[2 * N + k] = model_xyz[3 * j + 2];
            P[3 * N + k] = sp[(long)i * pt_stride];
            P[4 * N + k] = sp[(long)i * pt_stride + ch_stride];
            P[5 * N + k] = sp[(long)i * pt_stride + 2 * ch_stride];
            if (kIndexed) sel[(long)b * N + k] = i;
        }
        run += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) nsel[b] = run;
}

// The tail of the select kernels, by the whole block: hypothesis `win` with pose rt has won crop b.  The statistics of the first n
// compacted pairs of P within thr2 of rt, summed by block_sum; thread 0 writes the fit on them (pvn3d_eval_utils_kpls.py:108) to o,
// valid[b] = 1 and winner[b] = win.
__device__ __forceinline__ void refit_winner(const float* P, int N, int n, const float* rt, float thr2, double (*red)[16], int b, int win,
                                             float* o, uint8_t* valid, int32_t* winner)
{
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float ax = P[i], ay = P[N + i], az = P[2 * N + i], bx = P[3 * N + i], by = P[4 * N + i], bz = P[5 * N + i];
        if (residual2(rt, ax, ay, az, bx, by, bz) <= thr2) acc_pair(acc, ax, ay, az, bx, by, bz);
    }
    double tot[16];
    block_sum<16>(acc, red, tot);
    if (threadIdx.x == 0) {
        kabsch_fit(tot, o);
        valid[b] = 1;
        winner[b] = win;
    }
}

// The pair gate of an ICP iteration, over crop b by the whole block: pair(i, j, dd) for every point i that is selected and, when
// reject2 >= 0, not farther than the reject distance; j = its nearest vertex clamped into the model, dd = the squared distance clamped
// at 0.  (The loop with a callback and not a test that returns "keep": the kernels keep the control flow of the loop written out.)
template <typename F>
__device__ __forceinline__ void for_icp_pairs(const uint8_t* __restrict__ mask, const float* __restrict__ d2,
                                              const int32_t* __restrict__ nn, int b, int N, int M, float reject2, F pair)
{
    for (int i = threadIdx.x; i < N; i += 256) {
        if (!mask[(long)b * N + i]) continue;
        const float dd = fmaxf(d2[(long)b * N + i], 0.f);
        if (reject2 >= 0.f && !(dd <= reject2)) continue;
        int j = nn[(long)b * N + i];
        j = min(max(j, 0), M - 1);
        pair(i, j, dd);
    }
}

// One point-to-plane pair into the 30 sums { A = sum w J J^T (upper triangle, 21), g = sum w J r (6), S = sum w, L2 = sum w |x|^2,
// E = sum |r| }: x the point in the model frame, q the point of the plane, n its unit normal, r = n . (x - q), J = [x cross n ; n],
// w the Huber weight of r (delta <= 0: off).  The caller counts the pair.
__device__ __forceinline__ void acc_plane_pair(double* acc, double x, double y, double z, double nx, double ny, double nz, double qx,
                                               double qy, double qz, double delta)
{
    const double r = (nx * (x - qx) + ny * (y - qy)) + nz * (z - qz);
    const double ar = fabs(r);
    const double w = (delta <= 0.0 || ar <= delta) ? 1.0 : delta / ar;
    const double J[6] = {y * nz - z * ny, z * nx - x * nz, x * ny - y * nx, nx, ny, nz};
    int e = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const double wj = w * J[p];
#pragma unroll
        for (int q = p; q < 6; ++q) acc[e++] += wj * J[q];
        acc[21 + p] += wj * r;
    }
    acc[27] += w;
    acc[28] += w * ((x * x + y * y) + z * z);
    acc[29] += ar;
}

// Host side.  The refusals that the entries taking pairs share, under the entry's name `me`: `ptrs` is the entry's own NULL test,
// M < 0 an entry without a model, strides / max_B whether the entry tests the scene strides / the grid limit on B.
static inline int pair_entry_check(const char* me, bool ptrs, int B, int N, int M, bool strides, long scene_bstride, int pt_stride,
                                   int ch_stride, bool max_B)
{
    GDM_CHECK_ARG(ptrs, "%s: NULL pointer", me);
    if (M < 0) GDM_CHECK_ARG(B >= 1 && N >= 1, "%s: bad shape B=%d N=%d", me, B, N);
    else GDM_CHECK_ARG(B >= 1 && N >= 1 && M >= 1, "%s: bad shape B=%d N=%d M=%d", me, B, N, M);
    GDM_CHECK_ARG(!strides || (pt_stride >= 1 && ch_stride >= 1 && scene_bstride >= 0), "%s: bad scene strides", me);
    GDM_CHECK_ARG(!max_B || B <= 65535, "%s: B=%d > 65535", me, B);
    return 0;
}

// The next piece of a workspace: it starts `used` bytes into base and takes `bytes` rounded up to `align` (a power of two).
template <typename T>
static inline T* carve(void* base, size_t& used, size_t bytes, size_t align)
{
    T* piece = (T*)((char*)base + used);
    used += (bytes + align - 1) & ~(align - 1);
    return piece;
}

} // namespace
