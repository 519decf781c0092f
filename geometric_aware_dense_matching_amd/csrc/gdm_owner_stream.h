// The owner / stream skeleton of the training matching kernels, gfx950: circle_mm_kernel (gdm_circle.hip) and soft_coord_kernel
// (gdm_softcoord.hip).  A workgroup of 4 waves owns 128 items (32 per wave), each lane holding its item's whole K = 128 as
// split-bf16 fragments in registers; the other side is streamed through LDS in stages of 64 items (two 32-item sub-tiles): its
// packed rows for the S tile and, for the backward modes, its d-major copy for the second product.  Both operand forms are the
// buffers cm_pack_kernel writes.  What is here is the tile code only; argument structs, mode logic and the element-wise maths
// between the two products stay with the kernels.
// profiles/tile_helpers.md: what moving this code here changed in the kernels' instructions, and that it cost no time.
#pragma once
#include "gdm_common.h"

constexpr int ROWB = 512;                       // packed row: 128 bf16 hi | 128 bf16 lo
constexpr int OS_THREADS = 256;                 // 4 waves
constexpr int OS_OWN = 128;                     // owner items per workgroup (32 per wave)
constexpr int OS_ST = 64;                       // streamed items per LDS stage (two 32-item sub-tiles)
constexpr int TP_G = 128 * 64;                  // bytes of one plane of a d-major 32-item sub-tile in global memory
constexpr int TP_LSTRIDE = 80;                  // LDS bytes per d row of it (64 + 16 pad: conflict-free ds_read_b128)
constexpr int TP_L = 128 * TP_LSTRIDE;
constexpr int LDS_ROWS = OS_ST * ROWB;                       // 32 KiB
constexpr int LDS_TP = (OS_ST / 32) * 2 * TP_L;              // 40 KiB

__device__ __forceinline__ unsigned pack2(float a, float b)
{
    // plain casts: v_cvt_pk_bf16_f32 (round to nearest even, NaN stays NaN)
    const __bf16 x = (__bf16)a, y = (__bf16)b;
    return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
}
__device__ __forceinline__ float hi_of(float a) { return (float)(__bf16)a; }

__device__ __forceinline__ void split8(const float* v, gdm_u32x4& hi, gdm_u32x4& lo)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        hi[j] = pack2(v[2 * j], v[2 * j + 1]);
        lo[j] = pack2(v[2 * j] - hi_of(v[2 * j]), v[2 * j + 1] - hi_of(v[2 * j + 1]));
    }
}

// accumulator register q (0..7) of k-step ks, lane half h  ->  streamed index inside a 32-item sub-tile
__host__ __device__ __forceinline__ int acc_row(int ks, int h, int q) { return (q & 3) + 8 * (2 * ks + (q >> 2)) + 4 * h; }

// owner operand of the lane (item `own`, k half h): 8 k-steps x (hi, lo)
__device__ __forceinline__ void os_load_owner(const unsigned char* orows, int own, int h, gdm_u32x4 (&ohi)[8], gdm_u32x4 (&olo)[8])
{
    const unsigned char* r = orows + (long)own * ROWB + h * 16;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        ohi[s] = *reinterpret_cast<const gdm_u32x4*>(r + s * 32);
        olo[s] = *reinterpret_cast<const gdm_u32x4*>(r + 256 + s * 32);
    }
}

// stage st of the stream's packed rows -> the swizzled image at lrows (2048 chunks of 16 B, 8 per thread)
__device__ __forceinline__ void os_fill_rows(const unsigned char* srows, int st, unsigned char* lrows, int tid)
{
    const unsigned char* src = srows + (long)st * OS_ST * ROWB;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int gch = i * OS_THREADS + tid;
        *reinterpret_cast<gdm_u32x4*>(lrows + gdm_swz<ROWB>(gch >> 5, gch & 31)) = *reinterpret_cast<const gdm_u32x4*>(src + (long)gch * 16);
    }
}

// stage st of the stream's d-major tiles -> ltp: [sub-tile][plane hi | lo][128 d] rows of TP_LSTRIDE bytes
__device__ __forceinline__ void os_fill_tp(const unsigned char* stp, int st, unsigned char* ltp, int tid)
{
    const unsigned char* tsrc = stp + (long)st * (OS_ST / 32) * 2 * TP_G;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int gch = i * OS_THREADS + tid;           // (sub*2 + plane) * 512 + d * 4 + piece
        const int sp = gch >> 9, d = (gch >> 2) & 127, pc = gch & 3;
        *reinterpret_cast<gdm_u32x4*>(ltp + sp * TP_L + d * TP_LSTRIDE + pc * 16) = *reinterpret_cast<const gdm_u32x4*>(tsrc + (long)gch * 16);
    }
}

// S tile of one 32-item sub-tile: acc[i][j] = <stream_i, owner_j>, 24 MFMAs in the order hi*lo, lo*hi, hi*hi per k-step; row = the
// lane's row of the image at lrows (32 sub + j).  Register r of lane (j, h) <-> streamed item acc_row(r >> 3, h, r & 7), owner item j.
// (The row comes in as one value: given sub and j apart, the compiler hoists the sixteen swizzled addresses out of the stage loop
// and every circle_mm_kernel instance takes more registers.  soft_coord_kernel keeps its own text of this block: see there.)
__device__ __forceinline__ gdm_f32x16 os_s_tile(const unsigned char* lrows, int row, int h, const gdm_u32x4 (&ohi)[8], const gdm_u32x4 (&olo)[8])
{
    gdm_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const gdm_bf16x8 sh = __builtin_bit_cast(gdm_bf16x8, *reinterpret_cast<const gdm_u32x4*>(lrows + gdm_swz<ROWB>(row, 2 * s + h)));
        const gdm_bf16x8 sl = __builtin_bit_cast(gdm_bf16x8, *reinterpret_cast<const gdm_u32x4*>(lrows + gdm_swz<ROWB>(row, 16 + 2 * s + h)));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sh, __builtin_bit_cast(gdm_bf16x8, olo[s]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sl, __builtin_bit_cast(gdm_bf16x8, ohi[s]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sh, __builtin_bit_cast(gdm_bf16x8, ohi[s]), acc, 0, 0, 0);
    }
    return acc;
}

// out^T[d][j] += sum_i stream^T[d][i] G[i][j] over the four 32-channel blocks: G (in the S tile's register layout) goes STRAIGHT from
// the registers into the MFMA as its B operand; the d-major copy at ltp is packed in the k-order that layout dictates
__device__ __forceinline__ void os_second_product(const unsigned char* ltp, int sub, int j, int h, const float (&G)[16], gdm_f32x16 (&outacc)[4])
{
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        gdm_u32x4 gh, gl;
        split8(&G[8 * ks], gh, gl);
        const gdm_bf16x8 bgh = __builtin_bit_cast(gdm_bf16x8, gh), bgl = __builtin_bit_cast(gdm_bf16x8, gl);
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const unsigned char* p = ltp + (sub * 2) * TP_L + (db * 32 + j) * TP_LSTRIDE + (ks * 2 + h) * 16;
            const gdm_bf16x8 th = __builtin_bit_cast(gdm_bf16x8, *reinterpret_cast<const gdm_u32x4*>(p));
            const gdm_bf16x8 tl = __builtin_bit_cast(gdm_bf16x8, *reinterpret_cast<const gdm_u32x4*>(p + TP_L));
            outacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, bgl, outacc[db], 0, 0, 0);
            outacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tl, bgh, outacc[db], 0, 0, 0);
            outacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, bgh, outacc[db], 0, 0, 0);
        }
    }
}

// outacc[db][r] = grad[owner j][d = db*32 + acc_row(r)] -> the owner's 128-channel row `out`, as float4 (registers 4 q4 .. 4 q4 + 3 are
// four consecutive channels).  ADD: the lane adds `all` to every channel and `ch0` to channel 0.
template <bool ADD>
__device__ __forceinline__ void os_store_out(float* out, int h, const gdm_f32x16 (&outacc)[4], float all = 0.f, float ch0 = 0.f)
{
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int d = db * 32 + 8 * q4 + 4 * h;
            const gdm_f32x16& o = outacc[db];
            if (ADD) *reinterpret_cast<float4*>(out + d) = make_float4(o[4 * q4] + all + (d == 0 ? ch0 : 0.f), o[4 * q4 + 1] + all, o[4 * q4 + 2] + all, o[4 * q4 + 3] + all);
            else *reinterpret_cast<float4*>(out + d) = make_float4(o[4 * q4], o[4 * q4 + 1], o[4 * q4 + 2], o[4 * q4 + 3]);
        }
}

// Slices P of the stream in the grad-y mode (owner = the M vertices, stream = the R scene rows; the caller adds the P partial sums):
// ~3 workgroups per CU in flight, at most one slice per stage
static inline int os_bwd_parts(int R, int M)
{
    if (R < 1 || M < 1) return 0;
    const int vb = (M + 127) / 128, nst = (R + 127) / 128 * 128 / OS_ST;
    int P = (768 + vb - 1) / vb;
    if (P > nst) P = nst;
    return P < 1 ? 1 : P;
}
