// Consensus pose fit from pairwise-compatible correspondences, gfx950 (include/gdm.h THE CONSENSUS RULE).
//
// Two correct matches of a rigid object keep their distance, |p_i - p_j| = |q_i - q_j|.  The launches below count, for every selected
// pair of a crop, how many others agree with it (first and second order), pick seeds from those integer scores, fit one weighted
// hypothesis per seed and keep the one with the most inliers -- no draws, a fixed set of launches:
//   consensus_compact_kernel  one workgroup per crop: the selected correspondences (mask != 0) in point order as six fp32 planes
//                             (A = matched model vertex, B = scene point), the compact_pairs of gdm_pose_fit.h that
//                             ransac_compact_kernel runs, plus sel[k] = the point index of compacted k; score / degree start at -1
//   consensus_pairs_kernel    a 64-row tile of a crop's n x n compatibility BIT matrix: one lane per column, __ballot makes the word
//   consensus_score_kernel    deg_i = |row_i| and s_i = sum_{j in row_i} |row_i & row_j|: one lane per 64-bit word of a row (that is
//                             the N <= 4096 limit), 64 rows j staged in LDS once for the 16 rows i of a workgroup
//   consensus_seeds_kernel    one workgroup per crop: S masked arg-max steps over s, the covered set in LDS
//   consensus_fit_kernel      one workgroup per (seed, crop): the integer weights, the 16 weighted fp64 statistics in the fixed order
//                             of block_sum, the fit of gdm_kabsch_fit.inc, and that hypothesis' inlier count (ballot + popcount)
//   consensus_select_kernel   one workgroup per crop: the largest count (lowest t on ties) and the fp64 refit on its inliers
// No n x n float tensor exists: the workspace holds n x n bits per crop (512 KiB at N = 2048, 2 MiB at 4096).  No floating-point
// atomics; every sum has one order, so two launches give the same bytes.  The fit, the residual, the statistics and block_sum are
// the ones RANSAC and Kabsch use (gdm_pose_fit.h).
#include "gdm_pose_fit.h"

namespace {

typedef unsigned long long u64;

constexpr int MAX_N = 4096;             // one lane per 64-bit word of a bit row: 64 lanes x 64 bits
constexpr int MAX_SEEDS = 64;
constexpr int SCORE_ROWS_PER_WAVE = 4;  // consensus_score_kernel: the rows i a wave owns
constexpr int SCORE_ROWS = 4 * SCORE_ROWS_PER_WAVE;
constexpr int SCORE_SLOTS = 64 * (MAX_N / 64) / 256;                // words of a full 64-row tile per thread

// pts f32[B][6][N]: planes ax, ay, az, bx, by, bz of the selected pairs in point order; nsel i32[B] their number; sel i32[B][N] the
// point index of compacted k (k < nsel).  score / degree i32[B][N] are set to -1 here; consensus_score_kernel fills the selected ones.
__global__ __launch_bounds__(256) void consensus_compact_kernel(const float* __restrict__ scene_xyz, long scene_bstride, int pt_stride,
                                                                int ch_stride, const float* __restrict__ model_xyz,
                                                                const int32_t* __restrict__ best_idx, const uint8_t* __restrict__ mask,
                                                                int N, int M, float* __restrict__ pts, int32_t* __restrict__ nsel,
                                                                int32_t* __restrict__ sel, int32_t* __restrict__ score,
                                                                int32_t* __restrict__ degree)
{
    compact_pairs<true>(scene_xyz, scene_bstride, pt_stride, ch_stride, model_xyz, best_idx, mask, N, M, pts, nsel, sel, score, degree);
}

// bits u64[B][N][W], W = ceil(N / 64): bit (j & 63) of word j >> 6 of row i is C_ij (THE CONSENSUS RULE, step 1), for i, j < n; the
// bits of columns j >= n in the last word written are 0, words >= ceil(n / 64) and rows >= n are neither written nor read.
// Grid (ceil(N / 64), B): a workgroup holds 64 rows i in LDS; a wave takes every fourth 64-column block, one lane per column j.
__global__ __launch_bounds__(256) void consensus_pairs_kernel(const float* __restrict__ pts, const int32_t* __restrict__ nsel, int N, int W,
                                                              float tau2, u64* __restrict__ bits)
{
    __shared__ float srow[6][64];
    const int b = blockIdx.y;
    const int n = nsel[b];
    const int r0 = blockIdx.x * 64;
    if (r0 >= n) return;                                            // block-uniform
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* P = pts + (long)b * 6 * N;
    for (int e = threadIdx.x; e < 6 * 64; e += 256) {
        const int c = e >> 6, r = e & 63;
        srow[c][r] = r0 + r < n ? P[(long)c * N + r0 + r] : 0.f;
    }
    __syncthreads();
    const int nw = (n + 63) >> 6;
    u64* Bm = bits + (long)b * N * W;
    for (int cb = wave; cb < nw; cb += 4) {
        const int j = cb * 64 + lane;
        const bool inj = j < n;
        const int k = inj ? j : 0;
        const float qjx = P[k], qjy = P[N + k], qjz = P[2 * N + k], pjx = P[3 * N + k], pjy = P[4 * N + k], pjz = P[5 * N + k];
        u64 mine = 0;
        for (int ii = 0; ii < 64; ++ii) {
            float dx = srow[3][ii] - pjx, dy = srow[4][ii] - pjy, dz = srow[5][ii] - pjz;
            const float a2 = ((dx * dx) + dy * dy) + dz * dz;
            dx = srow[0][ii] - qjx; dy = srow[1][ii] - qjy; dz = srow[2][ii] - qjz;
            const float b2 = ((dx * dx) + dy * dy) + dz * dz;
            const float u = (a2 + b2) - tau2;
            const bool c = r0 + ii != j && (u <= 0.f || u * u <= (4.f * a2) * b2);
            const u64 bal = __ballot(inj && c);
            if (lane == ii) mine = bal;
        }
        if (r0 + lane < n) Bm[(long)(r0 + lane) * W + cb] = mine;
    }
}

// Word `l` of a 64-bit value that every lane holds its own copy of, as a wave-uniform value.
__device__ __forceinline__ u64 readlane64(u64 v, int l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}

// Step 2.  Grid (ceil(N / SCORE_ROWS), B).  Wave v of a workgroup owns SCORE_ROWS_PER_WAVE rows i; lane w keeps word w of each in a
// register.  Per 64 rows j: the tile goes to LDS once (dynamic, 65 rows of W words: row 64 stays zero), then for every owned row i
// the set bits of its word jt -- a wave-uniform value -- name the rows j to intersect, four at a time so that four LDS reads are in
// flight (a missing one reads the zero row).  Lanes >= nw hold 0 and read word nw - 1.
// sc / dg i32[B][N]: s and deg by compacted index (what the seed and fit kernels read); score / degree: the same per point.
__global__ __launch_bounds__(256) void consensus_score_kernel(const u64* __restrict__ bits, const int32_t* __restrict__ nsel,
                                                              const int32_t* __restrict__ sel, int N, int W, int32_t* __restrict__ sc,
                                                              int32_t* __restrict__ dg, int32_t* __restrict__ score,
                                                              int32_t* __restrict__ degree)
{
    extern __shared__ u64 tile[];                                   // [65][W]
    const int b = blockIdx.y;
    const int n = nsel[b];
    const int i0 = blockIdx.x * SCORE_ROWS;
    if (i0 >= n) return;                                            // block-uniform
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (n + 63) >> 6;
    const int lw = min(lane, nw - 1);
    const u64* Bm = bits + (long)b * N * W;
    u64 ri[SCORE_ROWS_PER_WAVE];
    int acc[SCORE_ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < SCORE_ROWS_PER_WAVE; ++r) {
        const int i = i0 + wave * SCORE_ROWS_PER_WAVE + r;
        ri[r] = (i < n && lane < nw) ? Bm[(long)i * W + lane] : 0ull;
        acc[r] = 0;
    }
    if (threadIdx.x < W) tile[64 * W + threadIdx.x] = 0ull;
    // Thread t moves words t, t + 256, ... of the 64 x nw tile: off[s] = row * W + word, the same in LDS and in the matrix.  The next
    // tile is fetched into registers while this one is worked on.
    int off[SCORE_SLOTS];
    {
        const int q = 256 / nw, rem = 256 - q * nw;
        int jj = threadIdx.x / nw, w = threadIdx.x - jj * nw;
#pragma unroll
        for (int k = 0; k < SCORE_SLOTS; ++k) {
            off[k] = jj < 64 ? jj * W + w : 0x7fffffff;
            jj += q; w += rem;
            if (w >= nw) { w -= nw; jj += 1; }
        }
    }
    u64 pre[SCORE_SLOTS];
    const auto fetch = [&](int jt) {
        const int lim = (n - jt * 64) * W;                          // rows j >= n hold zeros
        const u64* src = Bm + (long)jt * 64 * W;
#pragma unroll
        for (int k = 0; k < SCORE_SLOTS; ++k) pre[k] = off[k] < lim ? src[off[k]] : 0ull;
    };
    fetch(0);
    for (int jt = 0; jt < nw; ++jt) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SCORE_SLOTS; ++k)
            if (off[k] != 0x7fffffff) tile[off[k]] = pre[k];
        __syncthreads();
        if (jt + 1 < nw) fetch(jt + 1);
#pragma unroll
        for (int r = 0; r < SCORE_ROWS_PER_WAVE; ++r) {
            u64 cw = readlane64(ri[r], jt);                         // word jt of row i
            while (cw) {
                const int j0 = __builtin_ctzll(cw);
                cw &= cw - 1;
                const int j1 = cw ? __builtin_ctzll(cw) : 64;
                cw &= cw - 1;
                const int j2 = cw ? __builtin_ctzll(cw) : 64;
                cw &= cw - 1;
                const int j3 = cw ? __builtin_ctzll(cw) : 64;
                cw &= cw - 1;
                const u64 t0 = tile[j0 * W + lw], t1 = tile[j1 * W + lw], t2 = tile[j2 * W + lw], t3 = tile[j3 * W + lw];
                acc[r] += (__popcll(ri[r] & t0) + __popcll(ri[r] & t1)) + (__popcll(ri[r] & t2) + __popcll(ri[r] & t3));
            }
        }
    }
#pragma unroll
    for (int r = 0; r < SCORE_ROWS_PER_WAVE; ++r) {
        const int i = i0 + wave * SCORE_ROWS_PER_WAVE + r;
        const int s = wave_sum(acc[r]);
        const int d = wave_sum(__popcll(ri[r]));
        if (lane == 0 && i < n) {
            const int p = sel[(long)b * N + i];
            sc[(long)b * N + i] = s; dg[(long)b * N + i] = d;
            score[(long)b * N + p] = s; degree[(long)b * N + p] = d;
        }
    }
}

// Step 3: S sequential choices.  seedk i32[B][S] = the compacted index of seed t (-1: none), seed_idx the same as a point index.
__global__ __launch_bounds__(256) void consensus_seeds_kernel(const u64* __restrict__ bits, const int32_t* __restrict__ nsel,
                                                              const int32_t* __restrict__ sel, const int32_t* __restrict__ sc, int N,
                                                              int W, int S, int32_t* __restrict__ seedk, int32_t* __restrict__ seed_idx)
{
    __shared__ u64 covered[64];
    __shared__ int s_bs[4], s_bk[4];
    const int b = blockIdx.x;
    const int n = nsel[b];
    const int nw = (n + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64* Bm = bits + (long)b * N * W;
    if (threadIdx.x < 64) covered[threadIdx.x] = 0ull;
    __syncthreads();
    for (int t = 0; t < S; ++t) {
        int bs = 0, bk = 0x7fffffff;                                // only s > 0 can beat the start
        for (int k = threadIdx.x; k < n; k += 256) {
            if ((covered[k >> 6] >> (k & 63)) & 1ull) continue;
            const int s = sc[(long)b * N + k];
            if (s > bs || (s == bs && s > 0 && k < bk)) { bs = s; bk = k; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const int os = __shfl_xor(bs, off, 64), ok = __shfl_xor(bk, off, 64);
            if (os > bs || (os == bs && ok < bk)) { bs = os; bk = ok; }
        }
        if (lane == 0) { s_bs[wave] = bs; s_bk[wave] = bk; }
        __syncthreads();
        bs = s_bs[0]; bk = s_bk[0];
        for (int w = 1; w < 4; ++w)
            if (s_bs[w] > bs || (s_bs[w] == bs && s_bk[w] < bk)) { bs = s_bs[w]; bk = s_bk[w]; }
        const int g = bs > 0 ? bk : -1;                             // block-uniform
        if (g >= 0 && threadIdx.x < nw) {
            u64 v = covered[threadIdx.x] | Bm[(long)g * W + threadIdx.x];
            if (threadIdx.x == (g >> 6)) v |= 1ull << (g & 63);
            covered[threadIdx.x] = v;
        }
        if (threadIdx.x == 0) {
            seedk[(long)b * S + t] = g;
            seed_idx[(long)b * S + t] = g >= 0 ? sel[(long)b * N + g] : -1;
        }
        __syncthreads();
    }
}

// Steps 4 and 5 for hypothesis t = blockIdx.x of crop blockIdx.y: hyp f32[B][S][12], counts i32[B][S] (-1 with the sentinel pose: no
// seed, or fewer than 3 pairs of positive weight).
__global__ __launch_bounds__(256) void consensus_fit_kernel(const float* __restrict__ pts, const u64* __restrict__ bits,
                                                            const int32_t* __restrict__ nsel, const int32_t* __restrict__ dg,
                                                            const int32_t* __restrict__ seedk, int N, int W, int S, float thr2,
                                                            float* __restrict__ hyp, int32_t* __restrict__ counts)
{
    __shared__ u64 srow[64];
    __shared__ double red[4][16];
    __shared__ int cred[4];
    __shared__ float s_rt[12];
    const int t = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = nsel[b];
    const int nw = (n + 63) >> 6;
    const int g = seedk[(long)b * S + t];
    float* o = hyp + ((long)b * S + t) * 12;
    if (g < 0) {                                                    // block-uniform
        if (threadIdx.x == 0) { sentinel_pose(o); counts[(long)b * S + t] = -1; }
        return;
    }
    const u64* Bm = bits + (long)b * N * W;
    const float* P = pts + (long)b * 6 * N;
    if (threadIdx.x < 64) srow[threadIdx.x] = threadIdx.x < nw ? Bm[(long)g * W + threadIdx.x] : 0ull;
    __syncthreads();
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    int cnt = 0;
    for (int k = threadIdx.x; k < n; k += 256) {
        int w = 0;
        if (k == g) w = dg[(long)b * N + g];
        else if ((srow[k >> 6] >> (k & 63)) & 1ull) {
            const u64* rk = Bm + (long)k * W;
            for (int q = 0; q < nw; ++q) w += __popcll(srow[q] & rk[q]);
        }
        if (w > 0) {
            cnt += 1;
            acc_pair_w(acc, (double)w, P[k], P[N + k], P[2 * N + k], P[3 * N + k], P[4 * N + k], P[5 * N + k]);
        }
    }
    cnt = wave_sum(cnt);
    if (lane == 0) cred[wave] = cnt;                                // visible after block_sum's barrier
    double tot[16];
    block_sum<16>(acc, red, tot);
    const int n_pos = cred[0] + cred[1] + cred[2] + cred[3];
    if (n_pos < 3) {                                                // block-uniform
        if (threadIdx.x == 0) { sentinel_pose(o); counts[(long)b * S + t] = -1; }
        return;
    }
    if (threadIdx.x == 0) kabsch_fit(tot, s_rt);
    __syncthreads();
    float rt[12];
    for (int e = 0; e < 12; ++e) rt[e] = s_rt[e];
    if (threadIdx.x < 12) o[threadIdx.x] = rt[threadIdx.x];
    int c = 0;
    for (int i0 = wave * 64; i0 < n; i0 += 256) {
        const int i = i0 + lane;
        const bool in = i < n;
        const int k = in ? i : 0;
        c += __popcll(__ballot(in && residual2(rt, P[k], P[N + k], P[2 * N + k], P[3 * N + k], P[4 * N + k], P[5 * N + k]) <= thr2));
    }
    __syncthreads();                                                // cred is read above by every thread
    if (lane == 0) cred[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[(long)b * S + t] = cred[0] + cred[1] + cred[2] + cred[3];
}

// Step 6: the largest count wins (the lowest t on ties) and is refit, unweighted, on its inliers.
__global__ __launch_bounds__(256) void consensus_select_kernel(const float* __restrict__ pts, const int32_t* __restrict__ nsel,
                                                               const float* __restrict__ hyp, const int32_t* __restrict__ counts, int N,
                                                               int S, int min_points, float thr2, float* __restrict__ RT,
                                                               uint8_t* __restrict__ valid, int32_t* __restrict__ winner)
{
    __shared__ double red[4][16];
    const int b = blockIdx.x;
    const int n = nsel[b];
    float* o = RT + (long)b * 12;
    int bc = -1, bt = -1;
    for (int t = 0; t < S; ++t) {                                   // S <= 64: every thread walks the counts in order
        const int c = counts[(long)b * S + t];
        if (c > bc) { bc = c; bt = t; }
    }
    if (n < min_points || bc < min_points) {                        // block-uniform
        if (threadIdx.x == 0) { sentinel_pose(o); valid[b] = 0; winner[b] = -1; }
        return;
    }
    float rt[12];
    for (int e = 0; e < 12; ++e) rt[e] = hyp[((long)b * S + bt) * 12 + e];
    refit_winner(pts + (long)b * 6 * N, N, n, rt, thr2, red, b, bt, o, valid, winner);
}

struct ConsensusWs {
    float* pts;
    u64* bits;
    int32_t *nsel, *sel, *sc, *dg, *seedk;
    size_t bytes;
};

// Every piece is a multiple of 16 bytes, the bit matrix (the only 8-byte type) first after the planes.
ConsensusWs consensus_ws(void* base, int B, int N, int S)
{
    const size_t W = (size_t)(N + 63) / 64;
    const size_t bn = (size_t)B * N * sizeof(int32_t);
    ConsensusWs w;
    w.bytes = 0;
    w.pts = carve<float>(base, w.bytes, (size_t)B * 6 * N * sizeof(float), 16);
    w.bits = carve<u64>(base, w.bytes, (size_t)B * N * W * sizeof(u64), 16);
    w.sel = carve<int32_t>(base, w.bytes, bn, 16);
    w.sc = carve<int32_t>(base, w.bytes, bn, 16);
    w.dg = carve<int32_t>(base, w.bytes, bn, 16);
    w.nsel = carve<int32_t>(base, w.bytes, (size_t)B * sizeof(int32_t), 16);
    w.seedk = carve<int32_t>(base, w.bytes, (size_t)B * S * sizeof(int32_t), 16);
    return w;
}

} // namespace

extern "C" size_t gdm_consensus_workspace_bytes(int B, int N, int seeds)
{
    if (B < 1 || B > 65535 || N < 1 || N > MAX_N || seeds < 1 || seeds > MAX_SEEDS) return 0;
    return consensus_ws(nullptr, B, N, seeds).bytes;
}

extern "C" int gdm_consensus_pose_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* model_xyz,
                                      const int32_t* best_idx, const uint8_t* mask, int B, int N, int M, int seeds, float tau,
                                      float inlier_dist, int min_points, void* workspace, size_t workspace_bytes, float* RT,
                                      uint8_t* valid, int32_t* score, int32_t* degree, int32_t* seed_idx, float* hyp_RT, int32_t* counts,
                                      int32_t* winner, void* stream)
{
    int rc = pair_entry_check("gdm_consensus_pose_hip",
                              scene_xyz && model_xyz && best_idx && mask && workspace && RT && valid && score && degree && seed_idx &&
                                  hyp_RT && counts && winner,
                              B, N, M, true, scene_bstride, pt_stride, ch_stride, true);
    if (rc) return rc;
    GDM_CHECK_ARG(N <= MAX_N, "gdm_consensus_pose_hip: N=%d > %d (one lane per 64-bit word of a bit row)", N, MAX_N);
    GDM_CHECK_ARG(seeds >= 1 && seeds <= MAX_SEEDS, "gdm_consensus_pose_hip: seeds=%d not in [1,%d]", seeds, MAX_SEEDS);
    GDM_CHECK_ARG(tau > 0.f && tau < 1e18f, "gdm_consensus_pose_hip: tau=%g must be > 0", (double)tau);
    GDM_CHECK_ARG(inlier_dist > 0.f && inlier_dist < 1e18f, "gdm_consensus_pose_hip: inlier_dist=%g must be > 0", (double)inlier_dist);
    GDM_CHECK_ARG(min_points >= 3, "gdm_consensus_pose_hip: min_points=%d must be >= 3", min_points);
    const ConsensusWs w = consensus_ws(workspace, B, N, seeds);
    GDM_CHECK_ARG(workspace_bytes >= w.bytes, "gdm_consensus_pose_hip: workspace of %zu bytes, %zu needed", workspace_bytes, w.bytes);
    const hipStream_t s = (hipStream_t)stream;
    const int W = (N + 63) / 64, tiles = gdm_cdiv(N, 64);
    const float tau2 = tau * tau, thr2 = inlier_dist * inlier_dist;
    hipLaunchKernelGGL(consensus_compact_kernel, dim3(B), dim3(256), 0, s, scene_xyz, scene_bstride, pt_stride, ch_stride, model_xyz,
                       best_idx, mask, N, M, w.pts, w.nsel, w.sel, score, degree);
    if ((rc = gdm_launch_status("consensus_compact_kernel"))) return rc;
    hipLaunchKernelGGL(consensus_pairs_kernel, dim3(tiles, B), dim3(256), 0, s, w.pts, w.nsel, N, W, tau2, w.bits);
    if ((rc = gdm_launch_status("consensus_pairs_kernel"))) return rc;
    hipLaunchKernelGGL(consensus_score_kernel, dim3(gdm_cdiv(N, SCORE_ROWS), B), dim3(256), (size_t)65 * W * sizeof(u64), s, w.bits, w.nsel, w.sel, N, W, w.sc, w.dg, score, degree);
    if ((rc = gdm_launch_status("consensus_score_kernel"))) return rc;
    hipLaunchKernelGGL(consensus_seeds_kernel, dim3(B), dim3(256), 0, s, w.bits, w.nsel, w.sel, w.sc, N, W, seeds, w.seedk, seed_idx);
    if ((rc = gdm_launch_status("consensus_seeds_kernel"))) return rc;
    hipLaunchKernelGGL(consensus_fit_kernel, dim3(seeds, B), dim3(256), 0, s, w.pts, w.bits, w.nsel, w.dg, w.seedk, N, W, seeds, thr2,
                       hyp_RT, counts);
    if ((rc = gdm_launch_status("consensus_fit_kernel"))) return rc;
    hipLaunchKernelGGL(consensus_select_kernel, dim3(B), dim3(256), 0, s, w.pts, w.nsel, hyp_RT, counts, N, seeds, min_points, thr2, RT,
                       valid, winner);
    return gdm_launch_status("consensus_select_kernel");
}
