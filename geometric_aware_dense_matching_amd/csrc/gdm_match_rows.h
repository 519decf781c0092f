// The matching kernel's operand rows (gdm_match.hip): one descriptor of 128 channels, L2-normalised (x / max(|x|, 1e-12), F.normalize
// semantics) and stored as one row of 512 B -- 128 bf16 "hi" | 128 bf16 "lo" (GDM_MATCH_BF16X3) or 128 fp32 (GDM_MATCH_F32).
//
// One copy of the two loops that decide a row's bytes, for every kernel that writes such rows from a tile of 64 points held in LDS by a
// workgroup of 256 threads: pack_rows_tile (gdm_match.hip, the values come from global memory) and point_heads_kernel (gdm_heads.hip,
// the values are its own accumulators).  The callers differ only in where a value comes from.
//   1. part[w][lane] = gdm_rows_sumsq(w, ...)     wave w sums the squares of channels w, w + 4, ... of point `lane`, in that order
//   2. __syncthreads()
//   3. gdm_rows_store<PREC>(part, ...)            |x| = sqrtf((p0 + p1) + (p2 + p3)); thread = (point, 8-channel chunk)
#pragma once
#include "gdm_common.h"

constexpr int GDM_ROWS_D = 128;           // descriptor length
constexpr int GDM_ROWS_BYTES = 512;       // one packed row

// at(c): channel c of this lane's point.  settle(v): called on each group of eight values before they are used (a caller whose at()
// reads LDS retires the reads there, GDM_SETTLE_LDS; otherwise nothing).
template <class At, class Settle>
__device__ __forceinline__ float gdm_rows_sumsq(const int w, At&& at, Settle&& settle)
{
    float ss = 0.f;
#pragma unroll 1
    for (int c0 = w; c0 < GDM_ROWS_D; c0 += 32) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = at(c0 + 4 * j);
        settle(v);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
    }
    return ss;
}

// rows: the row of the tile's point 0; n_valid: points of the tile that exist (the others are not written); at(c, pl): channel c of
// the tile's point pl, from LDS.  Every thread recomputes the norm of the points it writes.
template <int PREC, class At>
__device__ __forceinline__ void gdm_rows_store(const float (*part)[64], const int n_valid, unsigned char* __restrict__ rows, At&& at)
{
#pragma unroll 1
    for (int it = 0; it < 4; ++it) {
        const int item = it * 256 + threadIdx.x;       // 64 points x 16 chunks of 8 channels
        const int ch = item & 15;
        const int pl = item >> 4;
        if (pl >= n_valid) continue;
        float p0 = part[0][pl], p1 = part[1][pl], p2 = part[2][pl], p3 = part[3][pl];
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = at(ch * 8 + j, pl);
        GDM_SETTLE_LDS("+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]),
                       "+v"(v[6]), "+v"(v[7]));
        const float nrm = sqrtf((p0 + p1) + (p2 + p3));
        const float inv_den = fmaxf(nrm, 1e-12f);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] / inv_den;
        unsigned char* row = rows + (long)pl * GDM_ROWS_BYTES;
        if (PREC == GDM_MATCH_BF16X3) {
            unsigned hi[4], lo[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                gdm_split2(v[2 * j], v[2 * j + 1], hi[j], lo[j]);
            }
            *reinterpret_cast<uint4*>(row + ch * 16) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
            *reinterpret_cast<uint4*>(row + 256 + ch * 16) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        } else {
            *reinterpret_cast<float4*>(row + ch * 32) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(row + ch * 32 + 16) = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
}
