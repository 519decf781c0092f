// DGCNN variant (BASELINE config 4) operators for gfx950:
//   * row-wise top-k of a dense score matrix  -- replaces `pairwise_distance.topk(k)` in
//     /root/reference/models/dgcnn.py:21-27 (dense [B,N,N] negative squared distances, k=16 cloud / k=20 mesh)
//   * edge feature  cat(x_j - x_i, x_i)       -- replaces get_graph_feature, dgcnn.py:30-56
// The dense score matrix itself stays a hipBLASLt GEMM through torch.matmul (same -xx - 2x^T x - xx^T
// formula as the reference, so near-tie behaviour follows the same arithmetic).
//
// top-k: one wave per row.  Lanes scan the row with stride 64 (coalesced 256-B reads), each keeps a sorted
// top-KMAX of its share in registers (branch-free shift insertion, as the xyz kNN kernel), and the 64
// lists are merged by k rounds of a shuffle arg-max.  Order: score descending, ties by ascending column.
#include "gdm_common.h"
#include <math.h>
#include <mutex>

namespace {

constexpr int TK_BLOCK = 256;
constexpr int IDX_EMPTY = 0x7fffffff;

// NEGDIST: `score` is the Gram matrix X^T X of one batch item per n rows and the ranked quantity is dgcnn.py:22-25's
// pairwise_distance[r][c] = ((-xx[c]) - (-2 * gram[r][c])) - xx[r], formed on the fly with torch's operations in torch's order
// (bit-identical), instead of four elementwise passes over the [B,n,n] matrix before the top-k.
//
// One wave per row; lane l scans columns l, l+64, ... into a PRIVATE sorted list of KP entries, then the 64 lists are merged
// by K rounds of wave arg-min.  A lane holds on average K/64 of the row's top K, so short private lists (KP = 4) almost always
// suffice and make the per-element insertion 4x cheaper; the row is exact iff no lane's KP-th entry is at least as good as
// the merged K-th -- otherwise (probability ~1e-4 per row on unordered data) the wave redoes the row with KP = KMAX.
template <int KP, bool NEGDIST>
__device__ __forceinline__ bool topk_row_pass(const float* __restrict__ s, const float* __restrict__ xb, float xr, int n, int K, int lane,
                                              long row, int32_t* __restrict__ idx, float* __restrict__ val, bool may_fail)
{
    float dl[KP];                                          // key = -score, ascending
    int il[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        dl[i] = INFINITY;
        il[i] = IDX_EMPTY;
    }
    for (int c = lane; c < n; c += 64) {
        const float d = NEGDIST ? -(((-xb[c]) - (-2.f * s[c])) - xr) : -s[c];
        if (d < dl[KP - 1]) {
            bool gt_hi = true;
#pragma unroll
            for (int i = KP - 1; i > 0; --i) {
                const bool gt_lo = dl[i - 1] > d;
                const float dn = gt_lo ? dl[i - 1] : (gt_hi ? d : dl[i]);
                const int in = gt_lo ? il[i - 1] : (gt_hi ? c : il[i]);
                dl[i] = dn;
                il[i] = in;
                gt_hi = gt_lo;
            }
            dl[0] = gt_hi ? d : dl[0];
            il[0] = gt_hi ? c : il[0];
        }
    }
    const float last = dl[KP - 1];                         // this lane's KP-th best (+inf while the list is not full)
    float outd = 0.f;                                      // round k's winner is kept by lane k until the row is known to be exact
    int outi = 0;
    float kth = INFINITY;
    for (int k = 0; k < K; ++k) {
        float bd = dl[0];
        int bi = il[0];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const float od = __shfl_xor(bd, m, 64);
            const int oi = __shfl_xor(bi, m, 64);
            if (od < bd || (od == bd && oi < bi)) {
                bd = od;
                bi = oi;
            }
        }
        if (dl[0] == bd && il[0] == bi) {
#pragma unroll
            for (int i = 0; i < KP - 1; ++i) {
                dl[i] = dl[i + 1];
                il[i] = il[i + 1];
            }
            dl[KP - 1] = INFINITY;
            il[KP - 1] = IDX_EMPTY;
        }
        if (lane == (k & 63)) {
            outd = bd;
            outi = bi;
        }
        kth = bd;
    }
    // a lane whose full private list ends at or before the merged K-th key may have dropped an element that belongs to the top K
    if (may_fail && __ballot(last <= kth && last < INFINITY) != 0ull) return false;
    if (lane < K) {
        idx[row * K + lane] = outi == IDX_EMPTY ? 0 : outi;
        if (val) val[row * K + lane] = -outd;
    }
    return true;
}

template <int KMAX, bool NEGDIST>
__global__ __launch_bounds__(TK_BLOCK) void topk_rows_kernel(const float* __restrict__ score, long rows, int n, int K,
                                                             int32_t* __restrict__ idx, float* __restrict__ val,
                                                             const float* __restrict__ xx = nullptr)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (TK_BLOCK / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                               // whole wave exits together
    const float* s = score + row * n;
    const float* xb = NEGDIST ? xx + (row / n) * n : nullptr;          // this batch item's squared norms
    const float xr = NEGDIST ? xb[row % n] : 0.f;
    constexpr int KP = KMAX >= 16 ? 4 : KMAX;
    if (KP < KMAX && n >= 64 * KP) {
        if (topk_row_pass<KP, NEGDIST>(s, xb, xr, n, K, lane, row, idx, val, true)) return;
    }
    (void)topk_row_pass<KMAX, NEGDIST>(s, xb, xr, n, K, lane, row, idx, val, false);
}

// out[b, c, i, k] = x[b,c,idx[b,i,k]] - x[b,c,i]   (c < C)
// out[b, C+c, i, k] = x[b,c,i]
__global__ __launch_bounds__(256) void edge_feature_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                           int C, int n, int K, float* __restrict__ out)
{
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * 8;
    const long nk = (long)n * K;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= nk) return;
    const int i = (int)(e / K);
    int j = idx[(long)b * nk + e];
    j = min(max(j, 0), n - 1);
    const int cend = min(c0 + 8, C);
    for (int c = c0; c < cend; ++c) {
        const float* xr = x + ((long)b * C + c) * n;
        const float xi = xr[i], xj = xr[j];
        out[((long)b * 2 * C + c) * nk + e] = xj - xi;
        out[((long)b * 2 * C + C + c) * nk + e] = xi;
    }
}

// grad_x[b,c,j] += g1 ; grad_x[b,c,i] += g2 - g1   (grad_x zeroed by the caller)
__global__ __launch_bounds__(256) void edge_feature_bwd_kernel(const float* __restrict__ go, const int32_t* __restrict__ idx,
                                                               int C, int n, int K, float* __restrict__ gx)
{
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * 8;
    const long nk = (long)n * K;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= nk) return;
    const int i = (int)(e / K);
    int j = idx[(long)b * nk + e];
    j = min(max(j, 0), n - 1);
    const int cend = min(c0 + 8, C);
    for (int c = c0; c < cend; ++c) {
        const float g1 = go[((long)b * 2 * C + c) * nk + e];
        const float g2 = go[((long)b * 2 * C + C + c) * nk + e];
        float* gr = gx + ((long)b * C + c) * n;
        atomicAdd(&gr[j], g1);
        atomicAdd(&gr[i], g2 - g1);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// feature_knn: k nearest neighbours in feature space without the [n,n] matrix.  A workgroup owns 32 rows of one item: two row groups
// of 16 (the MFMA's M) times S column splits = 2 S waves.  Per iteration the workgroup stages S column tiles of 64, channel-major in
// LDS (each channel row is contiguous in n: coalesced loads, 16-byte ones where n allows; the next iteration's loads are in flight
// during the products), and wave (row group, split s) takes tile S it + s: so one mesh (n = 8192, B = 1) still fills the chip, with
// no buffer beyond O(n).  A wave forms its 16 x 64 Gram tile on the fp32 MFMA (exact fp32 products, fp32 accumulation in channel
// order), the epilogue forms dgcnn.py:22-25's score in its order, and the selection keeps the idea of topk_row_pass: a row's 64
// scores of a tile sit in the 16 lanes (lane >> 4 == row / 4) x 4 accumulators, so each of those lanes keeps a PRIVATE sorted list of 8
// per row behind a bound on the row's K-th key, the 16 lists are merged by K rounds of a 16-lane arg-min, the S merged lists of a row
// are merged through LDS, and a row is exact iff no lane's 8th entry is at least as good as the row's final K-th.  Otherwise the
// workgroup is flagged and a second kernel sweeps it again with full-length lists (rare on unordered data).
constexpr int FK_ROWS = 32;                 // rows per workgroup: two row groups
constexpr int FK_SMAX = 4;                  // column splits per workgroup: 1, 2 or 4 (the launcher picks by the number of workgroups)
constexpr int FK_COLS = 64;
constexpr int FK_CK = 64;                   // channels per staged chunk
constexpr int FK_CMAX = 128;                // the row panel (all channels of the workgroup's rows) stays in LDS for the whole sweep
constexpr int FK_LDA = 48;                  // padded rows: stride mod 64 = 48 puts the four channel rows of an A operand read in distinct banks
constexpr int FK_LDB = 68;                  // 16-byte aligned rows; the shift of 4 banks per row keeps the 16-byte staging stores apart
constexpr int FK_PB = FK_CK * FK_COLS / 128;      // floats a thread stages per iteration: the two waves of a split stage its tile
constexpr int FK_KP = 8, FK_KMAX = 32;
constexpr int FK_MAXDEV = 64;
constexpr size_t FK_LDS_MAX = (size_t)(FK_SMAX * FK_CK * FK_LDB + FK_CMAX * FK_LDA) * sizeof(float);

__global__ __launch_bounds__(256) void feature_sqnorm_kernel(const float* __restrict__ x, long bstride, int C, int n, float* __restrict__ xx)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const float* xb = x + (long)blockIdx.y * bstride + c;
    float s = 0.f;
    for (int ch = 0; ch < C; ++ch) {
        const float v = xb[(long)ch * n];
        s += v * v;
    }
    xx[(long)blockIdx.y * n + c] = s;
}

template <int KP>
__device__ __forceinline__ void fk_insert(float (&dl)[KP], int (&il)[KP], float d, int c)
{
    if (d < dl[KP - 1]) {
        bool gt_hi = true;
#pragma unroll
        for (int i = KP - 1; i > 0; --i) {
            const bool gt_lo = dl[i - 1] > d;
            const float dn = gt_lo ? dl[i - 1] : (gt_hi ? d : dl[i]);
            const int in = gt_lo ? il[i - 1] : (gt_hi ? c : il[i]);
            dl[i] = dn;
            il[i] = in;
            gt_hi = gt_lo;
        }
        dl[0] = gt_hi ? d : dl[0];
        il[0] = gt_hi ? c : il[0];
    }
}

// Exchange within the 16 lanes of a DPP row without going through LDS: four involutions (neighbour, quad reversed, half row mirrored,
// row mirrored) that together reach every lane of the row, so four combine steps leave the row's reduction in all 16 lanes.
template <int CTRL>
__device__ __forceinline__ int fk_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ void fk_argmin_step(float& bd, int& bi)
{
    const float od = __int_as_float(fk_dpp<CTRL>(__float_as_int(bd)));
    const int oi = fk_dpp<CTRL>(bi);
    if (od < bd || (od == bd && oi < bi)) {                  // a total order on (key, column): both partners keep the same winner
        bd = od;
        bi = oi;
    }
}
__device__ __forceinline__ void fk_row_argmin(float& bd, int& bi)
{
    fk_argmin_step<0xB1>(bd, bi);                            // quad_perm [1,0,3,2]
    fk_argmin_step<0x1B>(bd, bi);                            // quad_perm [3,2,1,0]
    fk_argmin_step<0x141>(bd, bi);                           // row_half_mirror
    fk_argmin_step<0x140>(bd, bi);                           // row_mirror
}
__device__ __forceinline__ float fk_row_max(float t)
{
    t = fmaxf(t, __int_as_float(fk_dpp<0xB1>(__float_as_int(t))));
    t = fmaxf(t, __int_as_float(fk_dpp<0x1B>(__float_as_int(t))));
    t = fmaxf(t, __int_as_float(fk_dpp<0x141>(__float_as_int(t))));
    return fmaxf(t, __int_as_float(fk_dpp<0x140>(__float_as_int(t))));
}

__device__ __forceinline__ float fk_pick(const gdm_f32x4& v, int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3])); }

// One sweep over all columns for accumulator rows i0 .. i0 + NR - 1 of every wave, with private lists of KP.  Writes the rows'
// results and returns the mask (bit i) of the accumulator rows of this lane that may be inexact (always 0 unless may_fail).
// lds: S tiles [FK_CK][FK_LDB] (reused for the S merged lists of the 32 rows at the end), then the row panel [Cpad][FK_LDA].
template <int KP, int NR>
__device__ __forceinline__ unsigned fk_sweep(const float* __restrict__ xb, const float* __restrict__ xxb, int C, int n, int K, int r0, int i0,
                                             float* lds, float* kth_row, bool vec, int32_t* __restrict__ idx, float* __restrict__ val,
                                             bool may_fail)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane >> 4, lr = lane & 15;
    const int S = blockDim.x >> 7;
    const int rg = wave & 1, split = wave >> 1;             // waves 2 s, 2 s + 1 = threads 128 s .. 128 s + 127 stage and read tile s
    const int t7 = tid & 127;
    const int Cpad = (C + 3) & ~3;                           // channels past C are zeros (the C = 3 graph)
    const int nchunk = (Cpad + FK_CK - 1) / FK_CK;
    const int ntile = (n + FK_COLS - 1) / FK_COLS;
    const int total = ((ntile + S - 1) / S) * nchunk;
    float* Bs = lds + split * (FK_CK * FK_LDB);
    float* As = lds + S * (FK_CK * FK_LDB);
    const int bc = vec ? 4 * (t7 & 15) : (t7 & 63), bq = vec ? (t7 >> 4) : (t7 >> 6);          // staging roles, see below
    float pb[FK_PB];
    auto load = [&](int it) {
        const int itile = it / nchunk, q = it - itile * nchunk;
        const int c = (itile * S + split) * FK_COLS + bc;
        if (vec) {
            const unsigned cc = (unsigned)min(c, n - 4);
#pragma unroll
            for (int u = 0; u < FK_PB / 4; ++u) {
                const gdm_f32x4 v = *reinterpret_cast<const gdm_f32x4*>(xb + ((unsigned)(min(q * FK_CK + bq + 8 * u, C - 1) * n) + cc));
                pb[4 * u] = v[0], pb[4 * u + 1] = v[1], pb[4 * u + 2] = v[2], pb[4 * u + 3] = v[3];
            }
        } else {
            const unsigned cc = (unsigned)min(c, n - 1);
#pragma unroll
            for (int u = 0; u < FK_PB; ++u) pb[u] = xb[(unsigned)(min(q * FK_CK + bq + 2 * u, C - 1) * n) + cc];
        }
    };
    load(0);                                                 // the first tiles are in flight while the row panel is staged
    __syncthreads();                                         // a previous sweep has finished with the LDS
    // every address below is a valid one (clamped; 32-bit offsets from the uniform item base: the launcher checks C * n < 2^29) and
    // every load is unconditional -- a load under a select is turned into a branch with a wait behind it, one memory latency per
    // load; what lies outside the item is zeroed where the value is stored to LDS
    for (int e0 = tid; e0 < Cpad * FK_ROWS; e0 += 8 * (int)blockDim.x) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = min(e0 + u * (int)blockDim.x, Cpad * FK_ROWS - 1);
            v[u] = xb[(unsigned)(min(e >> 5, C - 1) * n) + (unsigned)min(r0 + (e & 31), n - 1)];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * (int)blockDim.x, ch = e >> 5, ar = e & 31;
            if (e < Cpad * FK_ROWS) As[ch * FK_LDA + ar] = (ch < C && r0 + ar < n) ? v[u] : 0.f;
        }
    }
    const int lrow = rg * 16 + lq * 4 + i0;                  // first of this lane's rows, within the workgroup
    float xr[NR], dl[NR][KP], lim[NR];                      // lim: what a candidate must beat = min(own list's last, bound on the row's K-th)
    int il[NR][KP];
#pragma unroll
    for (int ii = 0; ii < NR; ++ii) {
        xr[ii] = xxb[min(r0 + lrow + ii, n - 1)];
        lim[ii] = INFINITY;
#pragma unroll
        for (int i = 0; i < KP; ++i) {
            dl[ii][i] = INFINITY;
            il[ii][i] = IDX_EMPTY;
        }
    }
    // staging roles within the 128 threads of a split.  Scalar: column t7 & 63, channels (t7 >> 6) + 2 u.  16-byte (n % 4 == 0, aligned
    // base): column quad t7 & 15, channels (t7 >> 4) + 8 u.  Column 16 j + lr of the tile goes to position 4 lr + j of its LDS row.
    gdm_f32x4 acc[4];
    float xc[4];
    for (int it = 0; it < total; ++it) {
        const int itile = it / nchunk, q = it - itile * nchunk;
        const int tile = itile * S + split;
        __syncthreads();
        {
            const bool col_ok = tile * FK_COLS + bc < n;     // (a quad is inside or outside as a whole: n % 4 == 0 there)
            if (vec) {
                float* row0 = Bs + bq * FK_LDB + 4 * (bc & 15) + (bc >> 4);          // bc is a multiple of 4: columns bc + i sit 4 i further
                if ((tile + 1) * FK_COLS <= n && (q + 1) * FK_CK <= C) {             // the whole tile lies inside the item (uniform)
#pragma unroll
                    for (int u = 0; u < FK_PB / 4; ++u)
#pragma unroll
                        for (int i = 0; i < 4; ++i) row0[8 * u * FK_LDB + 4 * i] = pb[4 * u + i];
                } else {
#pragma unroll
                    for (int u = 0; u < FK_PB / 4; ++u) {
                        const bool ok = col_ok && q * FK_CK + bq + 8 * u < C;
#pragma unroll
                        for (int i = 0; i < 4; ++i) row0[8 * u * FK_LDB + 4 * i] = ok ? pb[4 * u + i] : 0.f;
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < FK_PB; ++u)
                    Bs[(bq + 2 * u) * FK_LDB + 4 * (bc & 15) + (bc >> 4)] = (col_ok && q * FK_CK + bq + 2 * u < C) ? pb[u] : 0.f;
            }
        }
        __syncthreads();
        if (it + 1 < total) load(it + 1);
        if (q == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[j] = gdm_f32x4{0.f, 0.f, 0.f, 0.f};
                xc[j] = xxb[min(tile * FK_COLS + 16 * j + lr, n - 1)];      // (columns past n get an infinite key below)
            }
        }
        const int steps = min(FK_CK, Cpad - q * FK_CK) >> 2;
        const float* ap = As + (q * FK_CK + lq) * FK_LDA + rg * 16 + lr;        // A[row lr][k lq], B[k lq][col lr]
        const float* bp = Bs + lq * FK_LDB + 4 * lr;        // the lane's four columns 16 j + lr are adjacent in LDS: one 16-byte read
        auto mfma_step = [&](float a, const gdm_f32x4& b) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[1], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[2], acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[3], acc[3], 0, 0, 0);
        };
        if (steps == FK_CK / 4) {                            // a whole chunk (uniform): fixed trip count, the next step's operands are
            float a = ap[0];                                 // read from LDS before this step's MFMAs are issued
            gdm_f32x4 b = *reinterpret_cast<const gdm_f32x4*>(bp);
#pragma unroll
            for (int s = 0; s < FK_CK / 4; ++s) {
                const int sn = s + 1 < FK_CK / 4 ? s + 1 : s;
                const float an = ap[4 * sn * FK_LDA];
                const gdm_f32x4 bn = *reinterpret_cast<const gdm_f32x4*>(bp + 4 * sn * FK_LDB);
                mfma_step(a, b);
                a = an;
                b = bn;
            }
        } else {
            for (int s = 0; s < steps; ++s) mfma_step(ap[4 * s * FK_LDA], *reinterpret_cast<const gdm_f32x4*>(bp + 4 * s * FK_LDB));
        }
        if (q == nchunk - 1) {
            // C/D layout: acc[j][i] = row 4 lq + i, column 16 j + lr of the tile
            const int cb = tile * FK_COLS + lr;
            const bool inside = (tile + 1) * FK_COLS <= n;   // uniform: no column of the tile lies past the item
#pragma unroll
            for (int ii = 0; ii < NR; ++ii) {
                float dj[4];
                unsigned pend = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float g = NR == 4 ? acc[j][ii] : fk_pick(acc[j], i0);
                    const float d = -(((-xc[j]) - (-2.f * g)) - xr[ii]);                           // key = -score, dgcnn.py:22-25's order
                    dj[j] = (inside || cb + 16 * j < n) ? d : INFINITY;
                    pend |= (dj[j] < lim[ii] ? 1u : 0u) << j;
                }
                // the few candidates that pass, in ascending column order: the loop runs as often as the busiest lane has candidates
                // (mostly once or not at all), instead of one insertion sequence per slot that any lane of the wave fills
                while (pend) {
                    const int j = __ffs(pend) - 1;
                    pend &= pend - 1;
                    fk_insert<KP>(dl[ii], il[ii], j == 0 ? dj[0] : (j == 1 ? dj[1] : (j == 2 ? dj[2] : dj[3])), cb + 16 * j);
                }
                lim[ii] = fminf(lim[ii], dl[ii][KP - 1]);
            }
            // a bound on the row's K-th key: the 16 lanes' best (K <= 16) or second best (K <= 32) entries are K distinct columns this
            // wave has seen, so a LATER candidate of this wave (a higher column: it loses every tie) that does not beat the largest of
            // them is not in the top K
            if ((itile & (itile + 1)) == 0) {                // after iterations 0, 1, 3, 7, 15, ...: the bound tightens ever more slowly
#pragma unroll
                for (int ii = 0; ii < NR; ++ii) {
                    lim[ii] = fminf(lim[ii], fk_row_max(K > 16 ? dl[ii][1] : dl[ii][0]));
                }
            }
        }
    }
    // merge the 16 lists of a row of this wave: K rounds of arg-min (ties: lower column) over the 16 lanes that share lane >> 4; round
    // k's winner goes to the split's list of the row in LDS (over the tiles, which every wave has finished reading)
    __syncthreads();
    float* md = lds;                                         // [S][32 rows][K] keys, then the same of columns
    int* mi = reinterpret_cast<int*>(lds) + S * FK_ROWS * K;
    float last[NR];
#pragma unroll
    for (int ii = 0; ii < NR; ++ii) {
        last[ii] = dl[ii][KP - 1];
        const int slot = (split * FK_ROWS + lrow + ii) * K;
        for (int k = 0; k < K; ++k) {
            float bd = dl[ii][0];
            int bi = il[ii][0];
            fk_row_argmin(bd, bi);
            if (dl[ii][0] == bd && il[ii][0] == bi) {
#pragma unroll
                for (int i = 0; i < KP - 1; ++i) {
                    dl[ii][i] = dl[ii][i + 1];
                    il[ii][i] = il[ii][i + 1];
                }
                dl[ii][KP - 1] = INFINITY;
                il[ii][KP - 1] = IDX_EMPTY;
            }
            if (lr == (k & 15)) {
                md[slot + k] = bd;
                mi[slot + k] = bi;
            }
        }
    }
    __syncthreads();
    // the S sorted lists of a row -> its K results: one thread per (row, accumulator row of this sweep), K steps of an S-way merge
    if (tid < FK_ROWS && (NR == 4 || (tid & 3) == i0)) {
        const long row = r0 + tid;
        int p[FK_SMAX] = {0, 0, 0, 0};
        float kd = INFINITY;
        for (int k = 0; k < K; ++k) {
            float bd = INFINITY;
            int bi = IDX_EMPTY, bs = 0;
#pragma unroll
            for (int s = 0; s < FK_SMAX; ++s) {
                if (s < S && p[s] < K) {
                    const float d = md[(s * FK_ROWS + tid) * K + p[s]];
                    const int c = mi[(s * FK_ROWS + tid) * K + p[s]];
                    if (d < bd || (d == bd && c < bi)) {
                        bd = d;
                        bi = c;
                        bs = s;
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < FK_SMAX; ++s) p[s] += (s == bs) ? 1 : 0;
            if (row < n) {
                idx[row * K + k] = bi == IDX_EMPTY ? 0 : bi;
                if (val) val[row * K + k] = -bd;
            }
            kd = bd;
        }
        kth_row[tid] = kd;
    }
    __syncthreads();
    // a lane whose full private list ends at or before the row's K-th key may have dropped an element of the top K
    unsigned fail = 0;
    if (may_fail) {
#pragma unroll
        for (int ii = 0; ii < NR; ++ii)
            if (last[ii] <= kth_row[lrow + ii] && last[ii] < INFINITY) fail |= 1u << (i0 + ii);
    }
    return fail;
}

__global__ __launch_bounds__(128 * FK_SMAX) void feature_knn_kernel(const float* __restrict__ x, long bstride, const float* __restrict__ xx, int C, int n,
                                                                    int K, int vec, int32_t* __restrict__ idx, float* __restrict__ val,
                                                                    int* __restrict__ redo)
{
    extern __shared__ __attribute__((aligned(16))) float fk_lds[];
    __shared__ float kth_row[FK_ROWS];
    __shared__ int any;
    const int b = blockIdx.y, r0 = blockIdx.x * FK_ROWS;
    idx += (long)b * n * K;
    if (val) val += (long)b * n * K;
    if (threadIdx.x == 0) any = 0;                            // (the sweep's barriers order this before the atomics below)
    const unsigned fail = fk_sweep<FK_KP, 4>(x + (long)b * bstride, xx + (long)b * n, C, n, K, r0, 0, fk_lds, kth_row, vec != 0, idx, val, K > FK_KP);
    if (K <= FK_KP) return;                                   // lists as long as K cannot overflow
    if (fail) atomicOr(&any, (int)fail);
    __syncthreads();
    if (threadIdx.x == 0) redo[b * gridDim.x + blockIdx.x] = any;          // bit i: accumulator row i of some wave may be inexact
}

// The exact redo of the workgroups feature_knn_kernel flagged (rare on unordered data: most workgroups leave at once): full-length
// lists, one accumulator row per sweep.  Rewrites all eight rows of that accumulator row -- both passes are exact where the first one
// did not flag, so the result does not depend on which rows were redone.  A kernel of its own so that the long lists do not set the
// register budget (and with it the occupancy) of the common pass.
__global__ __launch_bounds__(128 * FK_SMAX) void feature_knn_redo_kernel(const float* __restrict__ x, long bstride, const float* __restrict__ xx, int C,
                                                                         int n, int K, int vec, int32_t* __restrict__ idx, float* __restrict__ val,
                                                                         const int* __restrict__ redo)
{
    extern __shared__ __attribute__((aligned(16))) float fk_lds[];
    __shared__ float kth_row[FK_ROWS];
    const int b = blockIdx.y, r0 = blockIdx.x * FK_ROWS;
    const int f = redo[b * gridDim.x + blockIdx.x];           // uniform over the workgroup
    if (f == 0) return;
    idx += (long)b * n * K;
    if (val) val += (long)b * n * K;
#pragma unroll 1
    for (int i0 = 0; i0 < 4; ++i0)
        if ((f >> i0) & 1)
            (void)fk_sweep<FK_KMAX, 1>(x + (long)b * bstride, xx + (long)b * n, C, n, K, r0, i0, fk_lds, kth_row, vec != 0, idx, val, false);
}

// ---------------------------------------------------------------------------------------------------------------------------
// edge_block: one edge-convolution stage (dgcnn.py:108-120) without the [B,2C,n,k] edge tensor.  The stage's first convolution is linear
// in cat(x_j - x_i, x_i):  W cat(x_j - x_i, x_i) = W_a x_j + (W_b - W_a) x_i, so both products are formed per POINT by one per-point
// layer (pq f32[B,n,128] point-major: P = columns 0..63, Q = 64..127; a neighbour's row is one 256-byte read) and this kernel does, per
// point i and neighbour k:  h = lrelu(scale1 (P[idx[i,k]] + Q[i]) + shift1)  [-> h2 = lrelu(scale2 (W2 h) + shift2)]  -> max over k,
// written into channels [out_c0, out_c0 + 64) of out f32[B,out_C,n].  The second convolution runs on the fp32 MFMA with EDGES as the
// row dimension: a wave takes four points (4 K edges, 16 per MFMA tile), lane (edge lr, quarter lq) forms the edge's activations of
// channels 16 lq .. 16 lq + 15 as its A operands, and W2's matching fragments (64 registers) are read once per wave.
constexpr int EB_PTS = 64;                  // points per workgroup: four waves x four passes x four points
constexpr int EB_LDO = 65;

__device__ __forceinline__ float eb_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// the workgroup's 64 channels x 64 points from LDS to out[b, out_c0 + c, i0 + pt]: 256-byte rows along the points
__device__ __forceinline__ void eb_store_tile(const float* outs, float* __restrict__ out, int b, int out_C, int out_c0, int n, int i0)
{
    const int pt = threadIdx.x & 63, cq = threadIdx.x >> 6;
    if (i0 + pt < n)
        for (int c = cq; c < 64; c += 4) out[((long)b * out_C + out_c0 + c) * n + i0 + pt] = outs[c * EB_LDO + pt];
}

__global__ __launch_bounds__(256) void edge_block1_kernel(const float* __restrict__ pq, const int32_t* __restrict__ idx, const float* __restrict__ s1,
                                                          const float* __restrict__ t1, float slope, int n, int K, float* __restrict__ out,
                                                          int out_C, int out_c0)
{
    __shared__ float outs[64 * EB_LDO];
    const int b = blockIdx.y, i0 = blockIdx.x * EB_PTS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;             // lane = channel
    const float sc = s1[lane], sh = t1[lane];
    const float* pqb = pq + (long)b * n * 128;
    const int32_t* ib = idx + (long)b * n * K;
    for (int p = 0; p < 16; ++p) {
        const int pl = wave * 16 + p, i = i0 + pl;
        float m = -INFINITY;
        if (i < n) {                                                        // uniform over the wave
            const float q = pqb[(long)i * 128 + 64 + lane];
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                const int j = min(max(ib[(long)i * K + k], 0), n - 1);
                m = fmaxf(m, eb_lrelu(sc * (pqb[(long)j * 128 + lane] + q) + sh, slope));
            }
        }
        outs[lane * EB_LDO + pl] = m;
    }
    __syncthreads();
    eb_store_tile(outs, out, b, out_C, out_c0, n, i0);
}

__global__ __launch_bounds__(256) void edge_block2_kernel(const float* __restrict__ pq, const int32_t* __restrict__ idx, const float* __restrict__ s1,
                                                          const float* __restrict__ t1, const float* __restrict__ w2, const float* __restrict__ s2,
                                                          const float* __restrict__ t2, float slope, int n, int K, float* __restrict__ out,
                                                          int out_C, int out_c0)
{
    __shared__ float outs[64 * EB_LDO];
    const int b = blockIdx.y, i0 = blockIdx.x * EB_PTS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lq = lane >> 4, lr = lane & 15;
    // MFMA step s contracts channel 16 lq + s (any bijection of the 64 channels onto (step, lane >> 4) will do, as long as A and B
    // agree): then a lane's sixteen A values, its first-layer scale / shift and its W2 fragments are all 16-byte loads
    float wf[4][16], sc1[16], sh1[16], sc2[4], sh2[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float4 a = *reinterpret_cast<const float4*>(s1 + 16 * lq + 4 * m);
        const float4 c = *reinterpret_cast<const float4*>(t1 + 16 * lq + 4 * m);
        sc1[4 * m] = a.x, sc1[4 * m + 1] = a.y, sc1[4 * m + 2] = a.z, sc1[4 * m + 3] = a.w;
        sh1[4 * m] = c.x, sh1[4 * m + 1] = c.y, sh1[4 * m + 2] = c.z, sh1[4 * m + 3] = c.w;
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        sc2[jj] = s2[16 * jj + lr];
        sh2[jj] = t2[16 * jj + lr];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 w = *reinterpret_cast<const float4*>(w2 + (16 * jj + lr) * 64 + 16 * lq + 4 * m);       // W2[out 16 jj + lr][in 16 lq + 4 m ..]
            wf[jj][4 * m] = w.x, wf[jj][4 * m + 1] = w.y, wf[jj][4 * m + 2] = w.z, wf[jj][4 * m + 3] = w.w;
        }
    }
    const float* pqb = pq + (long)b * n * 128;
    const int32_t* ib = idx + (long)b * n * K;
    for (int t = 0; t < 4; ++t) {
        const int pbase = wave * 16 + 4 * t, ibase = i0 + pbase;
        const int np = min(4, n - ibase);                                   // uniform over the wave
        if (np <= 0) break;
        const int E = np * K;
        float mx[4][4];
#pragma unroll
        for (int P = 0; P < 4; ++P)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) mx[P][jj] = -INFINITY;
        for (int e0 = 0; e0 < E; e0 += 16) {
            const int eg = e0 + lr;
            const bool ev = eg < E;                                         // rows past the last edge contribute A = 0 and are masked below
            const int egc = ev ? eg : 0;
            const int p = egc / K, k = egc - p * K;
            const long i = ibase + p;
            const int j = min(max(ib[i * K + k], 0), n - 1);
            const float4* pr = reinterpret_cast<const float4*>(pqb + (long)j * 128 + 16 * lq);
            const float4* qr = reinterpret_cast<const float4*>(pqb + i * 128 + 64 + 16 * lq);
            float h[16];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float4 pv = pr[m], qv = qr[m];
                h[4 * m] = ev ? eb_lrelu(sc1[4 * m] * (pv.x + qv.x) + sh1[4 * m], slope) : 0.f;
                h[4 * m + 1] = ev ? eb_lrelu(sc1[4 * m + 1] * (pv.y + qv.y) + sh1[4 * m + 1], slope) : 0.f;
                h[4 * m + 2] = ev ? eb_lrelu(sc1[4 * m + 2] * (pv.z + qv.z) + sh1[4 * m + 2], slope) : 0.f;
                h[4 * m + 3] = ev ? eb_lrelu(sc1[4 * m + 3] * (pv.w + qv.w) + sh1[4 * m + 3], slope) : 0.f;
            }
            gdm_f32x4 acc[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[jj] = gdm_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(h[s], wf[jj][s], acc[jj], 0, 0, 0);
            // C/D layout: acc[jj][r] = edge e0 + 4 lq + r, channel 16 jj + lr
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ed = e0 + 4 * lq + r;
                const int pp = ed < E ? (ed >= K) + (ed >= 2 * K) + (ed >= 3 * K) : -1;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float v = eb_lrelu(sc2[jj] * acc[jj][r] + sh2[jj], slope);
#pragma unroll
                    for (int P = 0; P < 4; ++P) mx[P][jj] = pp == P ? fmaxf(mx[P][jj], v) : mx[P][jj];
                }
            }
        }
#pragma unroll
        for (int P = 0; P < 4; ++P)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                float m = mx[P][jj];
                m = fmaxf(m, __shfl_xor(m, 16, 64));
                m = fmaxf(m, __shfl_xor(m, 32, 64));
                if (lq == 0 && P < np) outs[(16 * jj + lr) * EB_LDO + pbase + P] = m;
            }
    }
    __syncthreads();
    eb_store_tile(outs, out, b, out_C, out_c0, n, i0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// edge_block in TRAINING mode: batch statistics over all B n K edges and a full backward, every pass recomputing its edges from pq, idx
// and per-channel numbers -- no buffer of O(B n K C) in either direction.  st f32[4][64] per BatchNorm = (scale = gamma rstd |
// shift = beta - mean scale | mean | rstd), cf f32[2][64] = (dbeta / E | dgamma / E).  Per-channel sums leave a workgroup as one fp64
// pair per channel (part[wg][64][2]); the caller folds the workgroups in fp64.
//   one convolution   edge_train1_kernel   lane = channel, a wave per point
//   two convolutions  edge_train2_kernel   the MFMA layout of edge_block2_kernel: a wave takes four points, 16 edges per tile
// Backward of the second convolution, per 16-edge tile of a wave: y1 and dy2 go through a 16 x 64 LDS tile each, because every product
// wants them in the other MFMA role than the one they were produced in (dy2: C/D of the forward product -> A of dh1 = dy2 W2;
// y1: A of the forward product -> the C/D positions, where it is the B operand of dW2 += dy2^T h1 and the mask / y_hat of dz1).
constexpr int ET_LD = 68;                   // 16-byte aligned rows, four banks apart
enum { ET_STATS = 0, ET_REDUCE = 1, ET_MID = 2, ET_SCATTER = 3 };

// the workgroup's 64 channels x 64 points of go[b, c, i0 + pt] into LDS (rows along the points: coalesced)
__device__ __forceinline__ void et_load_tile(float* gs, const float* __restrict__ go, int b, int n, int i0)
{
    const int pt = threadIdx.x & 63, cq = threadIdx.x >> 6;
    for (int c = cq; c < 64; c += 4) gs[c * EB_LDO + pt] = i0 + pt < n ? go[((long)b * 64 + c) * n + i0 + pt] : 0.f;
}

// red[wave][channel][2] -> part[wg][channel][2]
__device__ __forceinline__ void et_store_partials(double (*red)[64][2], double* __restrict__ part)
{
    __syncthreads();
    if (threadIdx.x < 64) {
        const long wg = (long)blockIdx.y * gridDim.x + blockIdx.x;
        const int c = threadIdx.x;
        part[(wg * 64 + c) * 2] = (red[0][c][0] + red[1][c][0]) + (red[2][c][0] + red[3][c][0]);
        part[(wg * 64 + c) * 2 + 1] = (red[0][c][1] + red[1][c][1]) + (red[2][c][1] + red[3][c][1]);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void edge_train1_kernel(const float* __restrict__ pq, const int32_t* __restrict__ idx, const float* __restrict__ st1,
                                                          const float* __restrict__ cf1, float slope, int n, int K, const float* __restrict__ go,
                                                          uint8_t* __restrict__ amax, double* __restrict__ part, float* __restrict__ dpq)
{
    __shared__ float gs[64 * EB_LDO];
    __shared__ double red[4][64][2];
    const int b = blockIdx.y, i0 = blockIdx.x * EB_PTS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;             // lane = channel
    float sc = 1.f, sh = 0.f, mu = 0.f, rs = 1.f, c0 = 0.f, c1 = 0.f;
    if (MODE != ET_STATS) {
        sc = st1[lane], sh = st1[64 + lane], mu = st1[128 + lane], rs = st1[192 + lane];
        et_load_tile(gs, go, b, n, i0);
        __syncthreads();
    }
    if (MODE == ET_SCATTER) c0 = cf1[lane], c1 = cf1[64 + lane];
    const float* pqb = pq + (long)b * n * 128;
    const int32_t* ib = idx + (long)b * n * K;
    double d0 = 0.0, d1 = 0.0;
    for (int p = 0; p < 16; ++p) {
        const int pl = wave * 16 + p, i = i0 + pl;
        if (i >= n) break;                                                  // uniform over the wave
        const float q = pqb[(long)i * 128 + 64 + lane];
        if (MODE == ET_STATS) {
            float s0 = 0.f, s1 = 0.f;                                       // fp32 over the K edges of a point, fp64 above
            for (int k = 0; k < K; ++k) {
                const int j = min(max(ib[(long)i * K + k], 0), n - 1);
                const float y = pqb[(long)j * 128 + lane] + q;
                s0 += y;
                s1 = fmaf(y, y, s1);
            }
            d0 += (double)s0;
            d1 += (double)s1;
        } else if (MODE == ET_REDUCE) {
            float hb = -INFINITY, yb = 0.f;
            int kb = 0;
            for (int k = 0; k < K; ++k) {
                const int j = min(max(ib[(long)i * K + k], 0), n - 1);
                const float y = pqb[(long)j * 128 + lane] + q;
                const float h = eb_lrelu(sc * y + sh, slope);
                if (h > hb) hb = h, yb = y, kb = k;                         // strict: the first arg-max
            }
            const float dz = gs[lane * EB_LDO + pl] * (sc * yb + sh > 0.f ? 1.f : slope);
            d0 += (double)dz;
            d1 += (double)(dz * ((yb - mu) * rs));
            amax[((long)b * n + i) * 64 + lane] = (uint8_t)kb;
        } else {
            const int a = amax[((long)b * n + i) * 64 + lane];
            const float g = gs[lane * EB_LDO + pl];
            float qs = 0.f;
            for (int k = 0; k < K; ++k) {
                const int j = min(max(ib[(long)i * K + k], 0), n - 1);
                const float y = pqb[(long)j * 128 + lane] + q;
                const float dz = k == a ? g * (sc * y + sh > 0.f ? 1.f : slope) : 0.f;
                const float dy = sc * (dz - c0 - (y - mu) * rs * c1);
                atomicAdd(&dpq[((long)b * n + j) * 128 + lane], dy);        // a neighbour's row: 256 contiguous bytes per wave
                qs += dy;
            }
            dpq[((long)b * n + i) * 128 + 64 + lane] = qs;
        }
    }
    if (MODE != ET_SCATTER) {
        red[wave][lane][0] = d0;
        red[wave][lane][1] = d1;
        et_store_partials(red, part);
    }
}

__device__ __forceinline__ void et_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MODE>
__global__ __launch_bounds__(256) void edge_train2_kernel(const float* __restrict__ pq, const int32_t* __restrict__ idx, const float* __restrict__ st1,
                                                          const float* __restrict__ w2, const float* __restrict__ st2, const float* __restrict__ cf1,
                                                          const float* __restrict__ cf2, float slope, int n, int K, const float* __restrict__ go,
                                                          uint8_t* __restrict__ amax, double* __restrict__ part, float* __restrict__ dwslab,
                                                          float* __restrict__ dpq)
{
    constexpr bool BWD = MODE == ET_MID || MODE == ET_SCATTER;
    __shared__ float gs[MODE == ET_STATS ? 1 : 64 * EB_LDO];
    __shared__ __attribute__((aligned(16))) float tiles[BWD ? 4 * 2 * 16 * ET_LD : 4];
    __shared__ double red[4][64][2];
    const int b = blockIdx.y, i0 = blockIdx.x * EB_PTS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lq = lane >> 4, lr = lane & 15;
    float wf[4][16], sc1[16], sh1[16], sc2[4], sh2[4], mu2[4], rs2[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float4 a = *reinterpret_cast<const float4*>(st1 + 16 * lq + 4 * m);
        const float4 c = *reinterpret_cast<const float4*>(st1 + 64 + 16 * lq + 4 * m);
        sc1[4 * m] = a.x, sc1[4 * m + 1] = a.y, sc1[4 * m + 2] = a.z, sc1[4 * m + 3] = a.w;
        sh1[4 * m] = c.x, sh1[4 * m + 1] = c.y, sh1[4 * m + 2] = c.z, sh1[4 * m + 3] = c.w;
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int c = 16 * jj + lr;
        sc2[jj] = MODE == ET_STATS ? 1.f : st2[c];
        sh2[jj] = MODE == ET_STATS ? 0.f : st2[64 + c];
        mu2[jj] = MODE == ET_STATS ? 0.f : st2[128 + c];
        rs2[jj] = MODE == ET_STATS ? 1.f : st2[192 + c];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 w = *reinterpret_cast<const float4*>(w2 + c * 64 + 16 * lq + 4 * m);                   // W2[out 16 jj + lr][in 16 lq + 4 m ..]
            wf[jj][4 * m] = w.x, wf[jj][4 * m + 1] = w.y, wf[jj][4 * m + 2] = w.z, wf[jj][4 * m + 3] = w.w;
        }
    }
    // backward only: W2 in the B role of dh1 = dy2 W2 (step s contracts output channel 16 lq + s), the first BatchNorm and the
    // coefficients at the C/D channels 16 jj + lr
    float wtf[BWD ? 4 : 1][16], sc1c[4], sh1c[4], mu1c[4], rs1c[4], c20[4], c21[4], c10[4], c11[4];
    if (BWD) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int c = 16 * jj + lr;
            sc1c[jj] = st1[c], sh1c[jj] = st1[64 + c], mu1c[jj] = st1[128 + c], rs1c[jj] = st1[192 + c];
            c20[jj] = cf2[c], c21[jj] = cf2[64 + c];
            c10[jj] = MODE == ET_SCATTER ? cf1[c] : 0.f;
            c11[jj] = MODE == ET_SCATTER ? cf1[64 + c] : 0.f;
#pragma unroll
            for (int s = 0; s < 16; ++s) wtf[jj][s] = w2[(16 * lq + s) * 64 + c];
        }
    }
    if (MODE != ET_STATS) {
        et_load_tile(gs, go, b, n, i0);
        __syncthreads();
    }
    float* ys = tiles + wave * (2 * 16 * ET_LD);                            // this wave's y1 tile, then its dy2 (later dy1) tile
    float* ds = ys + 16 * ET_LD;
    gdm_f32x4 dwacc[MODE == ET_MID ? 4 : 1][MODE == ET_MID ? 4 : 1];
    if (MODE == ET_MID) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) dwacc[a][bb] = gdm_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    double d0[4] = {0.0, 0.0, 0.0, 0.0}, d1[4] = {0.0, 0.0, 0.0, 0.0};
    const float* pqb = pq + (long)b * n * 128;
    const int32_t* ib = idx + (long)b * n * K;
    for (int t = 0; t < 4; ++t) {
        const int pbase = wave * 16 + 4 * t, ibase = i0 + pbase;
        const int np = min(4, n - ibase);                                   // uniform over the wave
        if (np <= 0) break;
        const int E = np * K;
        // per point P and C/D channel jj: the incoming gradient and the arg-max (backward), or the running arg-max (ET_REDUCE)
        float gP[4][4], hb[4][4], yb[4][4];
        int aP[4][4];
        if (MODE != ET_STATS) {
#pragma unroll
            for (int P = 0; P < 4; ++P)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    gP[P][jj] = gs[(16 * jj + lr) * EB_LDO + pbase + P];
                    hb[P][jj] = -INFINITY, yb[P][jj] = 0.f;
                    aP[P][jj] = (BWD && P < np) ? (int)amax[((long)b * n + ibase + P) * 64 + 16 * jj + lr] : 0;
                }
        }
        float qs[4] = {0.f, 0.f, 0.f, 0.f};
        for (int e0 = 0; e0 < E; e0 += 16) {
            const int eg = e0 + lr;
            const bool ev = eg < E;                                         // rows past the last edge contribute zeros and are masked below
            const int egc = ev ? eg : 0;
            const int p = egc / K, k = egc - p * K;
            const long i = ibase + p;
            const int j = min(max(ib[i * K + k], 0), n - 1);
            const float4* pr = reinterpret_cast<const float4*>(pqb + (long)j * 128 + 16 * lq);
            const float4* qr = reinterpret_cast<const float4*>(pqb + i * 128 + 64 + 16 * lq);
            float h[16];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float4 pv = pr[m], qv = qr[m];
                const float y0 = pv.x + qv.x, y1 = pv.y + qv.y, y2 = pv.z + qv.z, y3 = pv.w + qv.w;
                h[4 * m] = ev ? eb_lrelu(sc1[4 * m] * y0 + sh1[4 * m], slope) : 0.f;
                h[4 * m + 1] = ev ? eb_lrelu(sc1[4 * m + 1] * y1 + sh1[4 * m + 1], slope) : 0.f;
                h[4 * m + 2] = ev ? eb_lrelu(sc1[4 * m + 2] * y2 + sh1[4 * m + 2], slope) : 0.f;
                h[4 * m + 3] = ev ? eb_lrelu(sc1[4 * m + 3] * y3 + sh1[4 * m + 3], slope) : 0.f;
                if (BWD) *reinterpret_cast<float4*>(ys + lr * ET_LD + 16 * lq + 4 * m) = make_float4(y0, y1, y2, y3);
            }
            gdm_f32x4 acc[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[jj] = gdm_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(h[s], wf[jj][s], acc[jj], 0, 0, 0);
            // C/D layout: acc[jj][r] = edge e0 + 4 lq + r, channel 16 jj + lr
            if (MODE == ET_STATS) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    float s0 = 0.f, s1 = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (e0 + 4 * lq + r < E) {
                            s0 += acc[jj][r];
                            s1 = fmaf(acc[jj][r], acc[jj][r], s1);
                        }
                    d0[jj] += (double)s0;
                    d1[jj] += (double)s1;
                }
            } else if (MODE == ET_REDUCE) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ed = e0 + 4 * lq + r;
                    const int pp = ed < E ? (ed >= K) + (ed >= 2 * K) + (ed >= 3 * K) : -1;
                    const int kk = ed - pp * K;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const float v = eb_lrelu(sc2[jj] * acc[jj][r] + sh2[jj], slope);
#pragma unroll
                        for (int P = 0; P < 4; ++P) {
                            const bool up = pp == P && v > hb[P][jj];       // edges ascend within a lane: strict keeps the first
                            hb[P][jj] = up ? v : hb[P][jj];
                            yb[P][jj] = up ? acc[jj][r] : yb[P][jj];
                            aP[P][jj] = up ? kk : aP[P][jj];
                        }
                    }
                }
            } else {
                et_wave_sync();                                             // (the previous tile's reads of ds are done)
                float dy2[4][4];                                            // [jj][r]
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ed = e0 + 4 * lq + r;
                    const int pp = ed < E ? (ed >= K) + (ed >= 2 * K) + (ed >= 3 * K) : -1;
                    const int kk = ed - pp * K;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        float g = 0.f;
                        int a = -1;
#pragma unroll
                        for (int P = 0; P < 4; ++P) {
                            g = pp == P ? gP[P][jj] : g;
                            a = pp == P ? aP[P][jj] : a;
                        }
                        const float y2v = acc[jj][r];
                        const float dz2 = kk == a ? g * (sc2[jj] * y2v + sh2[jj] > 0.f ? 1.f : slope) : 0.f;
                        dy2[jj][r] = pp >= 0 ? sc2[jj] * (dz2 - c20[jj] - (y2v - mu2[jj]) * rs2[jj] * c21[jj]) : 0.f;
                        ds[(4 * lq + r) * ET_LD + 16 * jj + lr] = dy2[jj][r];
                    }
                }
                et_wave_sync();
                // y1 at the C/D positions, dy2 in the A role
                float yc[4][4], dsa[16];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) yc[jj][r] = ys[(4 * lq + r) * ET_LD + 16 * jj + lr];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float4 v = *reinterpret_cast<const float4*>(ds + lr * ET_LD + 16 * lq + 4 * m);
                    dsa[4 * m] = v.x, dsa[4 * m + 1] = v.y, dsa[4 * m + 2] = v.z, dsa[4 * m + 3] = v.w;
                }
                if (MODE == ET_MID) {
                    // dW2[out][in] += dy2[e][out] h1[e][in], the four edges 4 lq + r (lq = 0..3) of step r as the contraction
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float hc[4];
#pragma unroll
                        for (int bb = 0; bb < 4; ++bb) hc[bb] = eb_lrelu(sc1c[bb] * yc[bb][r] + sh1c[bb], slope);
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int bb = 0; bb < 4; ++bb)
                                dwacc[a][bb] = __builtin_amdgcn_mfma_f32_16x16x4f32(dy2[a][r], hc[bb], dwacc[a][bb], 0, 0, 0);
                    }
                }
                gdm_f32x4 dh[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) dh[jj] = gdm_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 16; ++s)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) dh[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsa[s], wtf[jj][s], dh[jj], 0, 0, 0);
                // dh[jj][r] = edge e0 + 4 lq + r, input channel 16 jj + lr
                if (MODE == ET_SCATTER) et_wave_sync();                     // every lane has read dy2: the tile takes dy1
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    float s0 = 0.f, s1 = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool valid = e0 + 4 * lq + r < E;
                        const float y = yc[jj][r];
                        const float dz1 = valid ? dh[jj][r] * (sc1c[jj] * y + sh1c[jj] > 0.f ? 1.f : slope) : 0.f;
                        const float yh = (y - mu1c[jj]) * rs1c[jj];
                        if (MODE == ET_MID) {
                            s0 += dz1;
                            s1 = fmaf(dz1, yh, s1);
                        } else {
                            ds[(4 * lq + r) * ET_LD + 16 * jj + lr] = valid ? sc1c[jj] * (dz1 - c10[jj] - yh * c11[jj]) : 0.f;
                        }
                    }
                    d0[jj] += (double)s0;
                    d1[jj] += (double)s1;
                }
                if (MODE == ET_SCATTER) {
                    et_wave_sync();
                    // lane = channel: a neighbour's row takes one 256-byte atomic per edge, dQ of the wave's own points is summed here
                    const int ne = min(16, E - e0);
                    for (int e = 0; e < ne; ++e) {
                        const int je = __shfl(j, e, 64);                    // lane e (lq = 0, lr = e) holds the edge's neighbour
                        const float v = ds[e * ET_LD + lane];
                        atomicAdd(&dpq[((long)b * n + je) * 128 + lane], v);
                        const int ed = e0 + e;
                        const int pp = (ed >= K) + (ed >= 2 * K) + (ed >= 3 * K);
#pragma unroll
                        for (int P = 0; P < 4; ++P) qs[P] += pp == P ? v : 0.f;
                    }
                }
            }
        }
        if (MODE == ET_REDUCE) {
#pragma unroll
            for (int P = 0; P < 4; ++P)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    float hv = hb[P][jj], yv = yb[P][jj];
                    int kv = aP[P][jj];
#pragma unroll
                    for (int m = 16; m <= 32; m <<= 1) {
                        const float ho = __shfl_xor(hv, m, 64), yo = __shfl_xor(yv, m, 64);
                        const int ko = __shfl_xor(kv, m, 64);
                        if (ho > hv || (ho == hv && ko < kv)) hv = ho, yv = yo, kv = ko;
                    }
                    if (lq == 0 && P < np) {
                        const float dz = gP[P][jj] * (sc2[jj] * yv + sh2[jj] > 0.f ? 1.f : slope);
                        d0[jj] += (double)dz;
                        d1[jj] += (double)(dz * ((yv - mu2[jj]) * rs2[jj]));
                        amax[((long)b * n + ibase + P) * 64 + 16 * jj + lr] = (uint8_t)kv;
                    }
                }
        }
        if (MODE == ET_SCATTER) {
#pragma unroll
            for (int P = 0; P < 4; ++P)
                if (P < np) dpq[((long)b * n + ibase + P) * 128 + 64 + lane] = qs[P];
        }
    }
    if (MODE != ET_SCATTER) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            double a = d0[jj], c = d1[jj];
            a += __shfl_xor(a, 16, 64), c += __shfl_xor(c, 16, 64);
            a += __shfl_xor(a, 32, 64), c += __shfl_xor(c, 32, 64);
            if (lq == 0) {
                red[wave][16 * jj + lr][0] = a;
                red[wave][16 * jj + lr][1] = c;
            }
        }
        et_store_partials(red, part);
    }
    if (MODE == ET_MID) {
        // the four waves' dW2 tiles are added in wave order through LDS (over the edge tiles, which no wave reads any more) and leave as
        // one 64 x 64 slab per workgroup: dwacc[a][bb][r] = output channel 16 a + 4 lq + r, input channel 16 bb + lr
        __syncthreads();
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int bb = 0; bb < 4; ++bb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float* slot = tiles + (16 * a + 4 * lq + r) * 64 + 16 * bb + lr;
                            *slot = w == 0 ? dwacc[a][bb][r] : *slot + dwacc[a][bb][r];
                        }
            }
            __syncthreads();
        }
        const long wg = (long)blockIdx.y * gridDim.x + blockIdx.x;
        for (int e = threadIdx.x; e < 64 * 64; e += 256) dwslab[wg * 4096 + e] = tiles[e];
    }
}

} // namespace

extern "C" int gdm_topk_rows_hip(const float* score, long rows, int n, int K, int32_t* idx, float* val, void* stream)
{
    GDM_CHECK_ARG(score && idx, "gdm_topk_rows_hip: NULL pointer");
    GDM_CHECK_ARG(rows >= 1 && n >= 1 && K >= 1 && K <= 32, "gdm_topk_rows_hip: bad shape rows=%ld n=%d K=%d", rows, n, K);
    dim3 grid(gdm_cdiv(rows, TK_BLOCK / 64));
    hipStream_t s = (hipStream_t)stream;
    if (K <= 8) hipLaunchKernelGGL((topk_rows_kernel<8, false>), grid, dim3(TK_BLOCK), 0, s, score, rows, n, K, idx, val, (const float*)nullptr);
    else if (K <= 16) hipLaunchKernelGGL((topk_rows_kernel<16, false>), grid, dim3(TK_BLOCK), 0, s, score, rows, n, K, idx, val, (const float*)nullptr);
    else hipLaunchKernelGGL((topk_rows_kernel<32, false>), grid, dim3(TK_BLOCK), 0, s, score, rows, n, K, idx, val, (const float*)nullptr);
    return gdm_launch_status("topk_rows_kernel");
}

extern "C" int gdm_topk_negdist_hip(const float* gram, const float* xx, int B, int n, int K, int32_t* idx, void* stream)
{
    GDM_CHECK_ARG(gram && xx && idx, "gdm_topk_negdist_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && n >= 1 && K >= 1 && K <= 32, "gdm_topk_negdist_hip: bad shape B=%d n=%d K=%d", B, n, K);
    const long rows = (long)B * n;
    dim3 grid(gdm_cdiv(rows, TK_BLOCK / 64));
    hipStream_t s = (hipStream_t)stream;
    float* nov = nullptr;
    if (K <= 8) hipLaunchKernelGGL((topk_rows_kernel<8, true>), grid, dim3(TK_BLOCK), 0, s, gram, rows, n, K, idx, nov, xx);
    else if (K <= 16) hipLaunchKernelGGL((topk_rows_kernel<16, true>), grid, dim3(TK_BLOCK), 0, s, gram, rows, n, K, idx, nov, xx);
    else hipLaunchKernelGGL((topk_rows_kernel<32, true>), grid, dim3(TK_BLOCK), 0, s, gram, rows, n, K, idx, nov, xx);
    return gdm_launch_status("topk_negdist_kernel");
}

extern "C" int gdm_edge_feature_hip(const float* x, const int32_t* idx, int B, int C, int n, int K, float* out, void* stream)
{
    GDM_CHECK_ARG(x && idx && out, "gdm_edge_feature_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && n >= 1 && K >= 1, "gdm_edge_feature_hip: bad shape");
    dim3 grid(gdm_cdiv((long)n * K, 256), gdm_cdiv(C, 8), B);
    hipLaunchKernelGGL(edge_feature_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, idx, C, n, K, out);
    return gdm_launch_status("edge_feature_kernel");
}

extern "C" int gdm_edge_feature_bwd_hip(const float* grad_out, const int32_t* idx, int B, int C, int n, int K, float* grad_x, void* stream)
{
    GDM_CHECK_ARG(grad_out && idx && grad_x, "gdm_edge_feature_bwd_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && n >= 1 && K >= 1, "gdm_edge_feature_bwd_hip: bad shape");
    dim3 grid(gdm_cdiv((long)n * K, 256), gdm_cdiv(C, 8), B);
    hipLaunchKernelGGL(edge_feature_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, grad_out, idx, C, n, K, grad_x);
    return gdm_launch_status("edge_feature_bwd_kernel");
}

extern "C" size_t gdm_feature_knn_workspace_bytes(int B, int n)
{
    if (B < 1 || n < 1) return 0;
    return ((size_t)B * n + (size_t)B * gdm_cdiv(n, FK_ROWS)) * 4;          // xx f32[B,n], then one redo flag per workgroup
}

extern "C" int gdm_feature_knn_hip(const float* x, long x_bstride, int B, int C, int n, int K, int splits, void* ws, size_t ws_bytes, int32_t* idx,
                                   float* val, void* stream)
{
    GDM_CHECK_ARG(x && ws && idx, "gdm_feature_knn_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && C <= FK_CMAX && n >= 1 && K >= 1 && K <= FK_KMAX,
                  "gdm_feature_knn_hip: bad shape B=%d C=%d (<= %d) n=%d K=%d (<= %d)", B, C, FK_CMAX, n, K, FK_KMAX);
    GDM_CHECK_ARG(splits == 0 || splits == 1 || splits == 2 || splits == 4, "gdm_feature_knn_hip: splits=%d not 0 (choose), 1, 2 or 4", splits);
    GDM_CHECK_ARG((long)C * n < (1L << 29), "gdm_feature_knn_hip: C * n = %ld: one item must stay below 2 GiB", (long)C * n);
    GDM_CHECK_ARG(x_bstride >= (long)C * n, "gdm_feature_knn_hip: batch stride %ld below C * n", x_bstride);
    GDM_CHECK_ARG(ws_bytes >= gdm_feature_knn_workspace_bytes(B, n), "gdm_feature_knn_hip: workspace of %zu bytes, %zu needed", ws_bytes,
                  gdm_feature_knn_workspace_bytes(B, n));
    hipStream_t s = (hipStream_t)stream;
    float* xx = (float*)ws;
    int* redo = (int*)ws + (size_t)B * n;
    {
        // more than 64 KiB of dynamic LDS needs the attribute, which holds per device: raised once for each device a thread of this
        // process launches on (before any capture: the first call on a device is an eager one)
        static std::mutex mu;
        static bool raised[FK_MAXDEV];
        int dev = 0;
        GDM_HIP(hipGetDevice(&dev));
        GDM_CHECK_ARG(dev >= 0 && dev < FK_MAXDEV, "gdm_feature_knn_hip: device %d", dev);
        std::lock_guard<std::mutex> lock(mu);
        if (!raised[dev]) {
            GDM_HIP(hipFuncSetAttribute((const void*)feature_knn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FK_LDS_MAX));
            GDM_HIP(hipFuncSetAttribute((const void*)feature_knn_redo_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FK_LDS_MAX));
            raised[dev] = true;
        }
    }
    const dim3 grid(gdm_cdiv(n, FK_ROWS), B);
    // column splits: as many as it takes to give the chip (256 CUs x 4 SIMDs) about two waves per SIMD
    const long wgs = (long)grid.x * B;
    const int S = splits ? splits : (wgs >= 2048 ? 1 : (wgs >= 512 ? 2 : 4));
    const int vec = (n % 4 == 0 && n >= 4 && ((uintptr_t)x & 15) == 0 && x_bstride % 4 == 0) ? 1 : 0;
    size_t tiles = (size_t)S * FK_CK * FK_LDB, lists = (size_t)2 * S * FK_ROWS * K;
    const size_t lds = ((tiles > lists ? tiles : lists) + (size_t)((C + 3) & ~3) * FK_LDA) * sizeof(float);
    hipLaunchKernelGGL(feature_sqnorm_kernel, dim3(gdm_cdiv(n, 256), B), dim3(256), 0, s, x, x_bstride, C, n, xx);
    hipLaunchKernelGGL(feature_knn_kernel, grid, dim3(128 * S), lds, s, x, x_bstride, (const float*)xx, C, n, K, vec, idx, val, redo);
    if (K > FK_KP)
        hipLaunchKernelGGL(feature_knn_redo_kernel, grid, dim3(128 * S), lds, s, x, x_bstride, (const float*)xx, C, n, K, vec, idx, val,
                           (const int*)redo);
    return gdm_launch_status("feature_knn_kernel");
}

extern "C" int gdm_edge_block_hip(const float* pq, const int32_t* idx, const float* scale1, const float* shift1, const float* w2,
                                  const float* scale2, const float* shift2, float slope, int B, int n, int K, float* out, int out_C, int out_c0,
                                  void* stream)
{
    GDM_CHECK_ARG(pq && idx && scale1 && shift1 && out, "gdm_edge_block_hip: NULL pointer");
    GDM_CHECK_ARG((w2 != nullptr) == (scale2 != nullptr) && (w2 != nullptr) == (shift2 != nullptr),
                  "gdm_edge_block_hip: the second convolution needs w2, scale2 and shift2 together");
    GDM_CHECK_ARG(B >= 1 && B <= 65535 && n >= 1 && K >= 1 && K <= 32, "gdm_edge_block_hip: bad shape B=%d n=%d K=%d", B, n, K);
    GDM_CHECK_ARG(out_c0 >= 0 && out_c0 + 64 <= out_C, "gdm_edge_block_hip: channels [%d, %d) outside the output's %d", out_c0, out_c0 + 64, out_C);
    GDM_CHECK_ARG((((uintptr_t)pq | (uintptr_t)scale1 | (uintptr_t)shift1 | (uintptr_t)w2) & 15) == 0,
                  "gdm_edge_block_hip: pq, scale1, shift1 and w2 must be 16-byte aligned");
    const dim3 grid(gdm_cdiv(n, EB_PTS), B);
    hipStream_t s = (hipStream_t)stream;
    if (w2)
        hipLaunchKernelGGL(edge_block2_kernel, grid, dim3(256), 0, s, pq, idx, scale1, shift1, w2, scale2, shift2, slope, n, K, out, out_C, out_c0);
    else
        hipLaunchKernelGGL(edge_block1_kernel, grid, dim3(256), 0, s, pq, idx, scale1, shift1, slope, n, K, out, out_C, out_c0);
    return gdm_launch_status("edge_block_kernel");
}

namespace {
bool et_shape_ok(int B, int n, int K) { return B >= 1 && B <= 65535 && n >= 1 && K >= 1 && K <= 32 && (long)B * n * 128 < (1L << 40); }
bool et_aligned(const void* a, const void* b, const void* c) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0; }
} // namespace

extern "C" long gdm_edge_train_groups(int B, int n)
{
    if (B < 1 || n < 1) return 0;
    return (long)B * gdm_cdiv(n, EB_PTS);
}

extern "C" int gdm_edge_stats_hip(const float* pq, const int32_t* idx, const float* st1, const float* w2, float slope, int B, int n, int K, double* part,
                                  void* stream)
{
    GDM_CHECK_ARG(pq && idx && part, "gdm_edge_stats_hip: NULL pointer");
    GDM_CHECK_ARG((w2 != nullptr) == (st1 != nullptr), "gdm_edge_stats_hip: the second convolution's statistics need st1 and w2 together");
    GDM_CHECK_ARG(et_shape_ok(B, n, K), "gdm_edge_stats_hip: bad shape B=%d n=%d K=%d", B, n, K);
    GDM_CHECK_ARG(et_aligned(pq, st1, w2), "gdm_edge_stats_hip: pq, st1 and w2 must be 16-byte aligned");
    const dim3 grid(gdm_cdiv(n, EB_PTS), B);
    hipStream_t s = (hipStream_t)stream;
    const float* nof = nullptr;
    uint8_t* nob = nullptr;
    float* now = nullptr;
    if (w2)
        hipLaunchKernelGGL(edge_train2_kernel<ET_STATS>, grid, dim3(256), 0, s, pq, idx, st1, w2, nof, nof, nof, slope, n, K, nof, nob, part, now, now);
    else
        hipLaunchKernelGGL(edge_train1_kernel<ET_STATS>, grid, dim3(256), 0, s, pq, idx, nof, nof, slope, n, K, nof, nob, part, now);
    return gdm_launch_status("edge_stats_kernel");
}

extern "C" int gdm_edge_bwd_reduce_hip(const float* pq, const int32_t* idx, const float* st1, const float* w2, const float* st2, float slope, int B, int n,
                                       int K, const float* grad_out, uint8_t* amax, double* part, void* stream)
{
    GDM_CHECK_ARG(pq && idx && st1 && grad_out && amax && part, "gdm_edge_bwd_reduce_hip: NULL pointer");
    GDM_CHECK_ARG((w2 != nullptr) == (st2 != nullptr), "gdm_edge_bwd_reduce_hip: the second convolution needs w2 and st2 together");
    GDM_CHECK_ARG(et_shape_ok(B, n, K), "gdm_edge_bwd_reduce_hip: bad shape B=%d n=%d K=%d", B, n, K);
    GDM_CHECK_ARG(et_aligned(pq, st1, w2), "gdm_edge_bwd_reduce_hip: pq, st1 and w2 must be 16-byte aligned");
    const dim3 grid(gdm_cdiv(n, EB_PTS), B);
    hipStream_t s = (hipStream_t)stream;
    const float* nof = nullptr;
    float* now = nullptr;
    if (w2)
        hipLaunchKernelGGL(edge_train2_kernel<ET_REDUCE>, grid, dim3(256), 0, s, pq, idx, st1, w2, st2, nof, nof, slope, n, K, grad_out, amax, part, now, now);
    else
        hipLaunchKernelGGL(edge_train1_kernel<ET_REDUCE>, grid, dim3(256), 0, s, pq, idx, st1, nof, slope, n, K, grad_out, amax, part, now);
    return gdm_launch_status("edge_bwd_reduce_kernel");
}

extern "C" int gdm_edge_bwd_mid_hip(const float* pq, const int32_t* idx, const float* st1, const float* w2, const float* st2, const float* cf2, float slope,
                                    int B, int n, int K, const float* grad_out, const uint8_t* amax, double* part, float* dw_slabs, void* stream)
{
    GDM_CHECK_ARG(pq && idx && st1 && w2 && st2 && cf2 && grad_out && amax && part && dw_slabs, "gdm_edge_bwd_mid_hip: NULL pointer");
    GDM_CHECK_ARG(et_shape_ok(B, n, K), "gdm_edge_bwd_mid_hip: bad shape B=%d n=%d K=%d", B, n, K);
    GDM_CHECK_ARG(et_aligned(pq, st1, w2), "gdm_edge_bwd_mid_hip: pq, st1 and w2 must be 16-byte aligned");
    const dim3 grid(gdm_cdiv(n, EB_PTS), B);
    const float* nof = nullptr;
    float* now = nullptr;
    hipLaunchKernelGGL(edge_train2_kernel<ET_MID>, grid, dim3(256), 0, (hipStream_t)stream, pq, idx, st1, w2, st2, nof, cf2, slope, n, K, grad_out,
                       const_cast<uint8_t*>(amax), part, dw_slabs, now);
    return gdm_launch_status("edge_bwd_mid_kernel");
}

extern "C" int gdm_edge_bwd_scatter_hip(const float* pq, const int32_t* idx, const float* st1, const float* cf1, const float* w2, const float* st2,
                                        const float* cf2, float slope, int B, int n, int K, const float* grad_out, const uint8_t* amax, float* grad_pq,
                                        void* stream)
{
    GDM_CHECK_ARG(pq && idx && st1 && cf1 && grad_out && amax && grad_pq, "gdm_edge_bwd_scatter_hip: NULL pointer");
    GDM_CHECK_ARG((w2 != nullptr) == (st2 != nullptr) && (w2 != nullptr) == (cf2 != nullptr),
                  "gdm_edge_bwd_scatter_hip: the second convolution needs w2, st2 and cf2 together");
    GDM_CHECK_ARG(et_shape_ok(B, n, K), "gdm_edge_bwd_scatter_hip: bad shape B=%d n=%d K=%d", B, n, K);
    GDM_CHECK_ARG(et_aligned(pq, st1, w2), "gdm_edge_bwd_scatter_hip: pq, st1 and w2 must be 16-byte aligned");
    const dim3 grid(gdm_cdiv(n, EB_PTS), B);
    hipStream_t s = (hipStream_t)stream;
    double* nod = nullptr;
    float* now = nullptr;
    uint8_t* am = const_cast<uint8_t*>(amax);
    if (w2)
        hipLaunchKernelGGL(edge_train2_kernel<ET_SCATTER>, grid, dim3(256), 0, s, pq, idx, st1, w2, st2, cf1, cf2, slope, n, K, grad_out, am, nod, now, grad_pq);
    else
        hipLaunchKernelGGL(edge_train1_kernel<ET_SCATTER>, grid, dim3(256), 0, s, pq, idx, st1, cf1, slope, n, K, grad_out, am, nod, grad_pq);
    return gdm_launch_status("edge_bwd_scatter_kernel");
}
