// N x M descriptor matching for gfx950 (MI355X): cosine similarity + row arg-max, optionally
// the materialised similarity matrix.
//
// Replaces (reference, /root/reference):
//   evaluator.py:87-93    F.normalize(rows) ; F.normalize(mesh, dim=0) ; matmul ; max(dim=1)
//   models/geoMatch.py:117-136 uses the same normalise + matmul with the (M+1)-column padded mesh
//
// Two kernels:
//   1. pack_rows_kernel   [R, D=128, n] channel-major fp32  ->  R*n packed rows of 512 B:
//        L2-normalise over D (x / max(|x|, 1e-12), F.normalize semantics) and store either
//          BF16X3: 128 bf16 "hi" | 128 bf16 "lo"   (|x - hi - lo| <= 2^-16 |x|)
//          F32   : 128 fp32
//        Transposes through LDS so that global reads are contiguous along n and global writes
//        are contiguous 512-B rows.
//   2. match_kernel<PREC, WRITE_SIM>  one workgroup = 4 waves = 128 scene rows; each wave keeps
//        its 32 rows' whole K=128 operand in registers (64 VGPRs) for the life of the kernel and
//        streams 64-column model tiles through a double-buffered, XOR-swizzled LDS image
//        (global -> registers before the MFMAs, registers -> LDS after them: issue-early /
//        write-late).  Products run on the matrix cores:
//          BF16X3: v_mfma_f32_32x32x16_bf16, three per k-step: hi*hi + hi*lo + lo*hi
//          F32   : v_mfma_f32_32x32x2_f32 (exact fp32 products, one rounding per FMA)
//        The epilogue keeps a running (max, first arg-max) per row in registers, reduces it
//        across the 32 lanes of a half-wave with shuffles, and (WRITE_SIM) stores the tile.
//        The M axis can be split over blockIdx.y; a small kernel merges the partial maxima.
//
// Roofline: materialised form moves 4D(BN+M) + 4BNM bytes; fused form 4D(BN+M)+8BN.
#include "gdm_common.h"
#include "gdm_match_rows.h"
#include <math.h>
#include <stdlib.h>

namespace {


constexpr int D = GDM_ROWS_D;          // descriptor length (config/lmo_cfg.py:125 feat_dim)
constexpr int ROW_BYTES = GDM_ROWS_BYTES;   // one packed row
constexpr int MT_ROWS = 128;           // scene rows per workgroup
constexpr int MT_COLS = 64;            // model columns per LDS tile
constexpr int TILE_BYTES = MT_COLS * ROW_BYTES;   // 32 KiB

// ------------------------------------------------------------------------------------------
// pack: [R, 128, n] -> R*n rows
// ------------------------------------------------------------------------------------------

// one block: 64 points (from p0) of row set r
template <int PREC>
__device__ __forceinline__ void pack_rows_tile(const float* __restrict__ x, int n, unsigned char* __restrict__ out, const int r, const int p0,
                                               float (*t)[65], float (*part)[64])
{
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int p = min(p0 + lane, n - 1);
    const float* xr = x + (long)r * D * n;
    part[w][lane] = gdm_rows_sumsq(w, [&](int c) {
        const float v = xr[(long)c * n + p];
        t[c][lane] = v;
        return v;
    }, [](float (&)[8]) {});
    __syncthreads();
    gdm_rows_store<PREC>(part, n - p0, out + ((long)r * n + p0) * ROW_BYTES, [&](int c, int pl) { return t[c][pl]; });
}

template <int PREC>
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ x, int n, unsigned char* __restrict__ out)
{
    __shared__ float t[D][65];
    __shared__ float part[4][64];
    pack_rows_tile<PREC>(x, n, out, blockIdx.y, blockIdx.x * 64, t, part);
}

// two independent packs in one launch (the scene descriptors [R1, 128, n1] and the model descriptors [R2, 128, n2] of one step):
// blockIdx.y < R1 walks the first, the rest the second; the same tile function, so the same bytes as two launches
template <int PREC>
__global__ __launch_bounds__(256) void pack_rows2_kernel(const float* __restrict__ x1, int R1, int n1, unsigned char* __restrict__ out1,
                                                         const float* __restrict__ x2, int n2, unsigned char* __restrict__ out2)
{
    __shared__ float t[D][65];
    __shared__ float part[4][64];
    const int p0 = blockIdx.x * 64;
    const int y = blockIdx.y;
    if (y < R1) {
        if (p0 < n1) pack_rows_tile<PREC>(x1, n1, out1, y, p0, t, part);
    } else {
        if (p0 < n2) pack_rows_tile<PREC>(x2, n2, out2, y - R1, p0, t, part);
    }
}

// ------------------------------------------------------------------------------------------
// match
// ------------------------------------------------------------------------------------------
// accumulator register reg (0..15) of a 32 x 32 MFMA result, lane half h -> its row, in a block that starts at row0 (the column is lane & 31)
__device__ __forceinline__ int acc_row(int row0, int reg, int h) { return row0 + (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// the scene operand of one lane: its row's 16 chunks (clamped to the last row), resident in registers
template <int PREC>
__device__ __forceinline__ void load_a_rows(const unsigned char* __restrict__ apk, int row, int R, int h, gdm_u32x4 (&a)[16])
{
    const unsigned char* arow = apk + (long)min(row, R - 1) * ROW_BYTES;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        int ch;
        if (PREC == GDM_MATCH_BF16X3) ch = (i < 8) ? (2 * i + h) : (16 + 2 * (i - 8) + h);   // hi[0..7], lo[0..7]
        else ch = 16 * h + i;                                                                // k = 64h + 4i..4i+3
        a[i] = *reinterpret_cast<const gdm_u32x4*>(arow + ch * 16);
    }
}

// acc[b][reg] of lane (lr, h) = <scene row acc_row(0, reg, h) of the wave (areg, as load_a_rows leaves it), model column c0 + 32 b> over
// the whole K = 128, the columns read from the swizzled image that starts base_off bytes into the dynamic LDS (c0 includes lr):
//   BF16X3: v_mfma_f32_32x32x16_bf16, three per k-step in the order hi*lo, lo*hi, hi*hi;  F32: v_mfma_f32_32x32x2_f32
// With NB = 2 the blocks alternate MFMA by MFMA, so that no MFMA waits for the one before it.  (The image is named by its offset:
// given a pointer, match_kernel comes out with other register counts.)
template <int PREC, int NB>
__device__ __forceinline__ void tile_product(int base_off, int c0, int h, const gdm_u32x4 (&areg)[16], gdm_f32x16 (&acc)[NB])
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned char* base = smem + base_off;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
    if (PREC == GDM_MATCH_BF16X3) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            gdm_bf16x8 bh[NB], bl[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                bh[b] = __builtin_bit_cast(gdm_bf16x8, *reinterpret_cast<const gdm_u32x4*>(base + gdm_swz<ROW_BYTES>(c0 + 32 * b, 2 * s + h)));
                bl[b] = __builtin_bit_cast(gdm_bf16x8, *reinterpret_cast<const gdm_u32x4*>(base + gdm_swz<ROW_BYTES>(c0 + 32 * b, 16 + 2 * s + h)));
            }
            const gdm_bf16x8 ah = __builtin_bit_cast(gdm_bf16x8, areg[s]);
            const gdm_bf16x8 al = __builtin_bit_cast(gdm_bf16x8, areg[8 + s]);
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[b], acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[b], acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[b], acc[b], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            gdm_u32x4 bv[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) bv[b] = *reinterpret_cast<const gdm_u32x4*>(base + gdm_swz<ROW_BYTES>(c0 + 32 * b, 16 * h + i));
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(areg[i][e]), __uint_as_float(bv[b][e]), acc[b], 0, 0, 0);
        }
    }
}

// running (max, first arg-max) of one row: columns arrive in ascending order, so strict '>' keeps the first maximum
__device__ __forceinline__ void running_max(float v, int col, bool ok, float& best, int& bidx)
{
    if (ok && v > best) {
        best = v;
        bidx = col;
    }
}

template <int PREC, bool WRITE_SIM>
__global__ __launch_bounds__(256) void match_kernel(const unsigned char* __restrict__ apk,   // [R] packed scene rows
                                                    const unsigned char* __restrict__ bpk,   // [M] packed model rows
                                                    int R, int M, int cols_per_split,
                                                    float* __restrict__ sim,                  // [R, M] or NULL
                                                    float* __restrict__ pval,                 // [splits, R]
                                                    int32_t* __restrict__ pidx)               // [splits, R]
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 2 x TILE_BYTES

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lr = lane & 31;        // row (A) / column (B) within a 32-block
    const int h = lane >> 5;         // k half

    const int row0 = blockIdx.x * MT_ROWS + wave * 32;
    const int split = blockIdx.y;
    const int col_begin = split * cols_per_split;
    const int col_end = min(col_begin + cols_per_split, M);
    const int ntiles = (col_end - col_begin + MT_COLS - 1) / MT_COLS;

    // ---- A operand: this lane's 16 chunks, resident for the whole kernel ----
    gdm_u32x4 areg[16];
    load_a_rows<PREC>(apk, row0 + lr, R, h, areg);

    float best[16];
    int bidx[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        best[i] = -INFINITY;
        bidx[i] = 0;
    }

    // ---- tile staging: 2048 chunks per tile, 8 per thread ----
    gdm_u32x4 stage[8];
    auto stage_load = [&](int tile) {
        const int c0 = col_begin + tile * MT_COLS;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int g = i * 256 + tid;
            const int col = g >> 5, ch = g & 31;
            const int gc = min(c0 + col, M - 1);
            stage[i] = *reinterpret_cast<const gdm_u32x4*>(bpk + (long)gc * ROW_BYTES + ch * 16);
        }
    };
    auto stage_store = [&](int buf) {
        unsigned char* base = smem + buf * TILE_BYTES;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int g = i * 256 + tid;
            const int col = g >> 5, ch = g & 31;
            *reinterpret_cast<gdm_u32x4*>(base + gdm_swz<ROW_BYTES>(col, ch)) = stage[i];
        }
    };

    if (ntiles > 0) {
        stage_load(0);
        stage_store(0);
    }
    __syncthreads();

    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        const bool has_next = tile + 1 < ntiles;
        if (has_next) stage_load(tile + 1);                 // global loads in flight under the MFMAs

        const int tcol0 = col_begin + tile * MT_COLS;

#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            gdm_f32x16 acc[1];
            const int col = cb * 32 + lr;
            tile_product<PREC, 1>(buf * TILE_BYTES, col, h, areg, acc);
            // ---- epilogue ----
            const int gcol = tcol0 + col;
            const bool col_ok = gcol < col_end;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float v = acc[0][reg];
                // running_max and acc_row restated: through the helpers match_kernel<*, true> comes out with other register counts
                if (col_ok && v > best[reg]) {              // strict: first maximum per lane (ascending columns)
                    best[reg] = v;
                    bidx[reg] = gcol;
                }
                if (WRITE_SIM) {
                    const int grow = row0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    if (col_ok && grow < R) sim[(long)grow * M + gcol] = v;
                }
            }
        }

        if (has_next) stage_store(buf ^ 1);
        __syncthreads();
    }

    // ---- reduce (max, lowest arg) across the 32 lanes of each half-wave ----
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        float v = best[reg];
        int ix = bidx[reg];
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) {
            const float ov = __shfl_xor(v, m, 64);
            const int oi = __shfl_xor(ix, m, 64);
            if (ov > v || (ov == v && oi < ix)) {
                v = ov;
                ix = oi;
            }
        }
        if (lr == 0) {
            const int grow = acc_row(row0, reg, h);
            if (grow < R) {
                pval[(long)split * R + grow] = v;
                pidx[(long)split * R + grow] = ix;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// match v2: model PANEL resident in LDS, scene row-blocks streamed through registers
// ------------------------------------------------------------------------------------------
// One workgroup = 8 waves (2 per SIMD) owns a panel of 256 model columns (128 KiB of packed rows, the
// whole LDS budget of a CU but for a sliver) for its lifetime and walks over row-blocks of 256 scene rows
// (32 per wave).  After the one-time panel fill there is NO barrier and no LDS write in the loop: a wave
// loads its 32 rows' operand (16 x 16 B per lane, straight to registers, next block prefetched), runs
// 8 column blocks x 24 (BF16X3) MFMAs against fragments read from the swizzled panel, and stores / arg-max
// reduces its own 32 x 256 outputs.  Tile stores of one wave overlap the MFMAs of its SIMD partner.
// Grid: blockIdx.x -> (g = bid % G, panel = bid / G): workgroups that read the same scene rows share
// `bid % 8`, i.e. (observed, speed only) one XCD's L2.
constexpr int PANEL_COLS = 256;
constexpr int PANEL_BYTES = PANEL_COLS * ROW_BYTES;     // 128 KiB
constexpr int V2_THREADS = 512;
constexpr int V2_ROWS = 256;                            // scene rows per workgroup iteration

// one-time panel fill at the start of the dynamic LDS: 256 columns x 32 chunks, 16 chunks per thread, coalesced 16-B loads; the columns
// of a partial last panel are clamped to M - 1
__device__ __forceinline__ void fill_panel(const unsigned char* bpk, int col0, int M, int tid)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int gi = i * V2_THREADS + tid;
        const int col = gi >> 5, ch = gi & 31;
        const int gc = min(col0 + col, M - 1);
        const gdm_u32x4 v = *reinterpret_cast<const gdm_u32x4*>(bpk + (long)gc * ROW_BYTES + ch * 16);
        *reinterpret_cast<gdm_u32x4*>(smem + gdm_swz<ROW_BYTES>(col, ch)) = v;
    }
}

// k-step s of a BF16X3 scene row that exists (no clamp): its hi and its lo chunk, reloaded inside the pipelined kernels' steps
__device__ __forceinline__ void load_a_step(const unsigned char* arow, int s, int h, gdm_u32x4 (&a)[16])
{
    a[s] = *reinterpret_cast<const gdm_u32x4*>(arow + (2 * s + h) * 16);
    a[8 + s] = *reinterpret_cast<const gdm_u32x4*>(arow + (16 + 2 * s + h) * 16);
}

// one halving step of the row butterfly for (max, lowest arg): the lane keeps the upper (up) or lower n of its 2n rows and merges
// the partner's values of them
template <int n>
__device__ __forceinline__ void halve_max(const float (&v)[2 * n], const int (&ix)[2 * n], float (&ov)[n], int (&oi)[n], bool up, int mask)
{
#pragma unroll
    for (int i = 0; i < n; ++i) {
        const float sv = up ? v[i] : v[i + n];
        const int si = up ? ix[i] : ix[i + n];
        const float pv = __shfl_xor(sv, mask, 64);
        const int pi = __shfl_xor(si, mask, 64);
        const float mv = up ? v[i + n] : v[i];
        const int mi = up ? ix[i + n] : ix[i];
        const bool take = pv > mv || (pv == mv && pi < mi);
        ov[i] = take ? pv : mv;
        oi[i] = take ? pi : mi;
    }
}

// lane bits 0..3 chose the upper half of the remaining row set at steps 1..4 of the butterfly: the register (row acc_row(row0, reg, h))
// whose result the lanes with (lane & 16) == 0 hold afterwards, reg = 8*b0 + 4*b1 + 2*b2 + b3
__device__ __forceinline__ int survivor_reg(int lane) { return ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3); }

// (max, lowest arg) across the 32 lanes of each half-wave, halving the row set every step: after step t each lane carries 16>>(t+1)
// rows, so 16+8+4+2 (+2) shuffles instead of 160; one lane per row writes.  GUARD: rows past R are not written (the pipelined
// kernels run only with R a multiple of the row block and need no guard)
template <bool GUARD = false>
__device__ __forceinline__ void finalize_rows(const float (&best)[16], const int (&bidx)[16], int lane, int h, int row0, int R,
                                              int panel, float* __restrict__ pval, int32_t* __restrict__ pidx)
{
    float v8[8], v4[4], v2[2], w1[1];
    int i8[8], i4[4], i2[2], j1[1];
    halve_max<8>(best, bidx, v8, i8, lane & 1, 1);
    halve_max<4>(v8, i8, v4, i4, lane & 2, 2);
    halve_max<2>(v4, i4, v2, i2, lane & 4, 4);
    halve_max<1>(v2, i2, w1, j1, lane & 8, 8);
    float v1 = w1[0];                                   // scalars from here on: left in the arrays, two registers of
    int i1 = j1[0];                                     // match_pipe_sim_kernel swap their names
    const float ov = __shfl_xor(v1, 16, 64);
    const int oi = __shfl_xor(i1, 16, 64);
    if (ov > v1 || (ov == v1 && oi < i1)) {
        v1 = ov;
        i1 = oi;
    }
    if ((lane & 16) == 0) {
        const int grow = acc_row(row0, survivor_reg(lane), h);
        if (GUARD && grow >= R) return;
        pval[(long)panel * R + grow] = v1;
        pidx[(long)panel * R + grow] = i1;
    }
}

template <int PREC, bool WRITE_SIM>
__global__ __launch_bounds__(V2_THREADS) void match_panel_kernel(const unsigned char* __restrict__ apk,
                                                                  const unsigned char* __restrict__ bpk,
                                                                  int R, int M, int G,
                                                                  float* __restrict__ sim,
                                                                  float* __restrict__ pval,      // [panels, R]
                                                                  int32_t* __restrict__ pidx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // PANEL_BYTES

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lr = lane & 31;
    const int h = lane >> 5;
    const int g = blockIdx.x % G;
    const int panel = blockIdx.x / G;
    const int col0 = panel * PANEL_COLS;
    const int ncols = min(PANEL_COLS, M - col0);

    fill_panel(bpk, col0, M, tid);
    __syncthreads();

    const int nrb = (R + V2_ROWS - 1) / V2_ROWS;
    gdm_u32x4 anext[16];
    if (g < nrb) load_a_rows<PREC>(apk, g * V2_ROWS + wave * 32 + lr, R, h, anext);

    for (int rb = g; rb < nrb; rb += G) {
        gdm_u32x4 areg[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) areg[i] = anext[i];
        if (rb + G < nrb) load_a_rows<PREC>(apk, (rb + G) * V2_ROWS + wave * 32 + lr, R, h, anext);
        const int row0 = rb * V2_ROWS + wave * 32;

        float best[16];
        int bidx[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            best[i] = -INFINITY;
            bidx[i] = 0;
        }

#pragma unroll 1
        for (int cp = 0; cp < PANEL_COLS / 64; ++cp) {
            gdm_f32x16 acc[2];
            const int c0 = cp * 64 + lr, c1 = c0 + 32;
            tile_product<PREC, 2>(0, c0, h, areg, acc);
            const int gc0 = col0 + c0, gc1 = col0 + c1;
            const bool ok0 = c0 < ncols, ok1 = c1 < ncols;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float v0 = acc[0][reg], v1 = acc[1][reg];
                running_max(v0, gc0, ok0, best[reg], bidx[reg]);
                running_max(v1, gc1, ok1, best[reg], bidx[reg]);
                if (WRITE_SIM) {
                    const int grow = acc_row(row0, reg, h);
                    if (grow < R) {
                        float* o = sim + (long)grow * M;
                        if (ok0) __builtin_nontemporal_store(v0, o + gc0);
                        if (ok1) __builtin_nontemporal_store(v1, o + gc1);
                    }
                }
            }
        }

        finalize_rows<true>(best, bidx, lane, h, row0, R, panel, pval, pidx);
    }
}

// ------------------------------------------------------------------------------------------
// match v3: v2's LDS-resident panel, software-pipelined inside the wave (BF16X3, full tiles only)
// ------------------------------------------------------------------------------------------
// PMC on v2 (profiles/r01_match_pmc.md): the MFMA pipe is busy 65 % (fused) / 39 % (materialised) of the SIMD's cycles; the two
// waves of a SIMD fall into phase (both issue MFMAs, then both run their ~130-instruction arg-max/store epilogue), so the pipe
// idles during every epilogue.  v3 removes the dependence on the partner wave:
//   * a wave's step t issues the 48 MFMAs of 64-column block t into one accumulator pair WHILE it drains block t-1 from the
//     other pair (running arg-max, stores), with the fragment reads of the next k-step (and of the next block's first k-step)
//     in flight; sched_group_barrier pins the interleave MFMA : ds_read : VALU : store, one scheduling region per step;
//   * the MFMA operand roles are swapped (srcA = model columns from the LDS panel, srcB = scene rows from registers), so a
//     lane holds 16 columns of ONE scene row per accumulator: the running (max, arg) is a single register pair per lane, the
//     row-block reduction is one shuffle, and the tile goes out as dwordx4 stores (4 consecutive columns per lane; plain
//     stores, merged to full lines in L2 -- tools/micro/store_pattern.hip: 5.95 TB/s for this pattern, non-temporal 1.8);
//   * the next row block's scene operand is prefetched into a second register set at the start of the row block, i.e. ahead of
//     that row block's stores in vmcnt order (loads issued behind ~100 stores wait for all of them).
// Requires R % 256 == 0 and M % 256 == 0 (no per-lane predication, so every step is one basic block); other shapes run v2.
// Same products, same accumulation order as v2: bit-identical results.
struct BFrag { gdm_u32x4 h0, l0, h1, l1; };

__device__ __forceinline__ BFrag read_bfrag(const unsigned char* smem, int c0, int s, int h)
{
    BFrag f;
    f.h0 = *reinterpret_cast<const gdm_u32x4*>(smem + gdm_swz<ROW_BYTES>(c0, 2 * s + h));
    f.l0 = *reinterpret_cast<const gdm_u32x4*>(smem + gdm_swz<ROW_BYTES>(c0, 16 + 2 * s + h));
    f.h1 = *reinterpret_cast<const gdm_u32x4*>(smem + gdm_swz<ROW_BYTES>(c0 + 32, 2 * s + h));
    f.l1 = *reinterpret_cast<const gdm_u32x4*>(smem + gdm_swz<ROW_BYTES>(c0 + 32, 16 + 2 * s + h));
    return f;
}

// (max, first arg-max) of the 32 values a lane holds for its row in one 64-column block, as a tournament: codes are
// compile-time constants at the leaves, every node takes its right child only if strictly greater (lower column wins ties).
// code = 16*acc + reg; column within the block = (reg&3) + 8*(reg>>2) + 32*acc (+ 4*h), ascending in code for a fixed lane.
__device__ __forceinline__ void block_argmax(const gdm_f32x16& p0, const gdm_f32x16& p1, float& bm, int& bc)
{
    // four independent scan chains over ascending code ranges (8 values each), merged left to right
    float m[4];
    int c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const gdm_f32x16& p = (j < 2) ? p0 : p1;
        const int r0 = (j & 1) * 8;
        m[j] = p[r0];
        c[j] = j * 8;
#pragma unroll
        for (int i = 1; i < 8; ++i) {
            const float v = p[r0 + i];
            const bool t = v > m[j];
            m[j] = t ? v : m[j];
            c[j] = t ? j * 8 + i : c[j];
        }
    }
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const bool t = m[j] > m[0];
        m[0] = t ? m[j] : m[0];
        c[0] = t ? c[j] : c[0];
    }
    bm = m[0];
    bc = c[0];
}

// One pipeline step: MFMAs of column block CP into (n0, n1) | drain (p0, p1) = column block PCP of row `prow`.
//   fr        in: fragments of (CP, k-step 0); out: fragments of ((CP+1)%4, k-step 0)
//   PREFETCH  : after k-step s, reload areg[s], areg[8+s] with the NEXT row block's operand (their last use in this row block)
//   DRAIN     : false only for the very first step of a workgroup (nothing to drain yet)
// acc[reg] of lane (lr, h) = sim[row lr][column (reg&3) + 8*(reg>>2) + 4*h of the 32-column block]
template <int CP, int PCP, bool PREFETCH, bool DRAIN>
__device__ __forceinline__ void pipe_step(const unsigned char* smem, int lr, int h, gdm_u32x4 (&areg)[16],
                                          BFrag& fr, gdm_f32x16& n0, gdm_f32x16& n1, const gdm_f32x16& p0, const gdm_f32x16& p1,
                                          float& best, int& bcode, const unsigned char* __restrict__ arow_next)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        n0[i] = 0.f;
        n1[i] = 0.f;
    }
    const int c0 = CP * 64 + lr;
    const int c0n = ((CP + 1) & 3) * 64 + lr;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const BFrag nx = (s < 7) ? read_bfrag(smem, c0, s + 1, h) : read_bfrag(smem, c0n, 0, h);
        const gdm_bf16x8 ah = __builtin_bit_cast(gdm_bf16x8, areg[s]);
        const gdm_bf16x8 al = __builtin_bit_cast(gdm_bf16x8, areg[8 + s]);
        const gdm_bf16x8 bh0 = __builtin_bit_cast(gdm_bf16x8, fr.h0), bl0 = __builtin_bit_cast(gdm_bf16x8, fr.l0);
        const gdm_bf16x8 bh1 = __builtin_bit_cast(gdm_bf16x8, fr.h1), bl1 = __builtin_bit_cast(gdm_bf16x8, fr.l1);
        n0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl0, ah, n0, 0, 0, 0);
        n1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl1, ah, n1, 0, 0, 0);
        n0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh0, al, n0, 0, 0, 0);
        n1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh1, al, n1, 0, 0, 0);
        n0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh0, ah, n0, 0, 0, 0);
        n1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh1, ah, n1, 0, 0, 0);
        if (PREFETCH) load_a_step(arow_next, s, h, areg);
        fr = nx;
    }
    if (DRAIN) {
        float lbest;
        int lcode;
        block_argmax(p0, p1, lbest, lcode);
        const bool take = lbest > best;                    // earlier blocks hold lower columns: strict '>' keeps the first maximum
        best = take ? lbest : best;
        bcode = take ? lcode + PCP * 32 : bcode;
    }
    // interleave: every MFMA is followed by a fragment read and a slice of the epilogue (one pipeline = one sync id per step)
#pragma unroll
    for (int i = 0; i < 48; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, CP);
        if (i < 32) __builtin_amdgcn_sched_group_barrier(0x100, 1, CP);
        if (PREFETCH && (i % 6) == 5) __builtin_amdgcn_sched_group_barrier(0x020, 2, CP);
        if (DRAIN) __builtin_amdgcn_sched_group_barrier(0x002, 2, CP);
    }
    __builtin_amdgcn_sched_barrier(0);          // one scheduling region per step: the interleave pipeline is matched per region
}

__global__ __launch_bounds__(V2_THREADS) void match_pipe_kernel(const unsigned char* __restrict__ apk,
                                                                 const unsigned char* __restrict__ bpk,
                                                                 int R, int M, int G,
                                                                 float* __restrict__ sim,
                                                                 float* __restrict__ pval,      // [panels, R]
                                                                 int32_t* __restrict__ pidx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // PANEL_BYTES

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31;
    const int h = lane >> 5;
    const int g = blockIdx.x % G;
    const int panel = blockIdx.x / G;
    const int col0 = panel * PANEL_COLS;

    // fill_panel (without the clamp) and load_a_step restated here and below: through the helpers match_pipe_kernel, which the
    // headline step runs, comes out with its instructions in another order
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int gi = i * V2_THREADS + tid;
        const int col = gi >> 5, ch = gi & 31;
        const gdm_u32x4 v = *reinterpret_cast<const gdm_u32x4*>(bpk + (long)(col0 + col) * ROW_BYTES + ch * 16);
        *reinterpret_cast<gdm_u32x4*>(smem + gdm_swz<ROW_BYTES>(col, ch)) = v;
    }
    __syncthreads();

    const int nrb = R / V2_ROWS;
    if (g >= nrb) return;
    gdm_u32x4 areg[16];
    {
        const unsigned char* arow = apk + (long)(g * V2_ROWS + wave * 32 + lr) * ROW_BYTES;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            areg[s] = *reinterpret_cast<const gdm_u32x4*>(arow + (2 * s + h) * 16);
            areg[8 + s] = *reinterpret_cast<const gdm_u32x4*>(arow + (16 + 2 * s + h) * 16);
        }
    }
    float best = -INFINITY;
    int bcode = 0;
    gdm_f32x16 a0, a1, b0, b1;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        b0[i] = 0.f;
        b1[i] = 0.f;
    }
    BFrag fr = read_bfrag(smem, lr, 0, h);

    // step 0 of the first row block: nothing to drain
    pipe_step<0, 0, false, false>(smem, lr, h, areg, fr, a0, a1, b0, b1, best, bcode, apk);

    for (int rb = g; rb < nrb; rb += G) {
        const int row0 = rb * V2_ROWS + wave * 32;                        // uniform
        const bool has_next = rb + G < nrb;
        const int nrow = (has_next ? (rb + G) * V2_ROWS : rb * V2_ROWS) + wave * 32 + lr;
        const unsigned char* arow_next = apk + (long)nrow * ROW_BYTES;
        pipe_step<1, 0, false, true>(smem, lr, h, areg, fr, b0, b1, a0, a1, best, bcode, arow_next);
        pipe_step<2, 1, false, true>(smem, lr, h, areg, fr, a0, a1, b0, b1, best, bcode, arow_next);
        pipe_step<3, 2, true, true>(smem, lr, h, areg, fr, b0, b1, a0, a1, best, bcode, arow_next);
        if (has_next) {
            pipe_step<0, 3, false, true>(smem, lr, h, areg, fr, a0, a1, b0, b1, best, bcode, arow_next);
        } else {
            float lbest;
            int lcode;
            block_argmax(b0, b1, lbest, lcode);
            const bool take = lbest > best;
            best = take ? lbest : best;
            bcode = take ? lcode + 96 : bcode;
        }
        // row-block result: code -> column, merge the two half-waves (lower column wins ties), one lane per row writes
        {
            int ix = col0 + ((bcode & 3) | (((bcode >> 2) & 3) << 3) | ((bcode >> 4) << 5)) + 4 * h;
            float v = best;
            const float ov = __shfl_xor(v, 32, 64);
            const int oi = __shfl_xor(ix, 32, 64);
            if (ov > v || (ov == v && oi < ix)) {
                v = ov;
                ix = oi;
            }
            if (h == 0) {
                pval[(long)panel * R + row0 + lr] = v;
                pidx[(long)panel * R + row0 + lr] = ix;
            }
        }
        best = -INFINITY;
        bcode = 0;
    }
}

// Materialised form of v3: original operand roles (lane = column, register = row), so one dword store instruction covers
// 2 rows x 128 contiguous bytes and may stay non-temporal; the swapped layout's 16-byte pieces need write-back merging in L2
// and lose under load (347 vs 256 us).  Running (max, arg) per register, v2's butterfly per row block.
// Steps of 32 columns (one accumulator in flight, one draining): 24 MFMAs | 16 values drained per step.
struct BFrag1 { gdm_u32x4 h, l; };

__device__ __forceinline__ BFrag1 read_bfrag1(const unsigned char* smem, int c, int s, int h)
{
    BFrag1 f;
    f.h = *reinterpret_cast<const gdm_u32x4*>(smem + gdm_swz<ROW_BYTES>(c, 2 * s + h));
    f.l = *reinterpret_cast<const gdm_u32x4*>(smem + gdm_swz<ROW_BYTES>(c, 16 + 2 * s + h));
    return f;
}

template <int CP, int PCP, bool RELOAD, bool DRAIN>
__device__ __forceinline__ void pipe_step_sim(const unsigned char* smem, int lr, int h, gdm_u32x4 (&areg)[16], BFrag1& fr,
                                              gdm_f32x16& n, const gdm_f32x16& p, float (&best)[16], int (&bidx)[16], int pgc,
                                              float* __restrict__ pbase, unsigned pvoff, long M,
                                              const unsigned char* __restrict__ arow_next)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) n[i] = 0.f;
    const int c = CP * 32 + lr;
    const int cn = ((CP + 1) & 7) * 32 + lr;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const BFrag1 nx = (s < 7) ? read_bfrag1(smem, c, s + 1, h) : read_bfrag1(smem, cn, 0, h);
        const gdm_bf16x8 ah = __builtin_bit_cast(gdm_bf16x8, areg[s]);
        const gdm_bf16x8 al = __builtin_bit_cast(gdm_bf16x8, areg[8 + s]);
        const gdm_bf16x8 bh = __builtin_bit_cast(gdm_bf16x8, fr.h), bl = __builtin_bit_cast(gdm_bf16x8, fr.l);
        n = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, n, 0, 0, 0);
        n = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, n, 0, 0, 0);
        n = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, n, 0, 0, 0);
        if (RELOAD) load_a_step(arow_next, s, h, areg);
        fr = nx;
    }
    if (DRAIN) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const float v = p[reg];
            // running_max restated (here and in the kernel's last drain) as selects: through the helper's branch match_pipe_sim_kernel,
            // which the headline step runs when the matrix is asked for, comes out with other instructions
            const bool t = v > best[reg];
            best[reg] = t ? v : best[reg];
            bidx[reg] = t ? pgc : bidx[reg];
            float* o = pbase + (long)acc_row(0, reg, 0) * M + PCP * 32;     // uniform row base, per-lane 32-bit offset
            __builtin_nontemporal_store(v, o + pvoff);
        }
    }
#pragma unroll
    for (int i = 0; i < 24; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, CP);
        if (i < 16) __builtin_amdgcn_sched_group_barrier(0x100, 1, CP);
        if (DRAIN) __builtin_amdgcn_sched_group_barrier(0x002, 2, CP);
        if (DRAIN && i >= 4 && i < 20) __builtin_amdgcn_sched_group_barrier(0x040, 1, CP);
    }
    __builtin_amdgcn_sched_barrier(0);
}

__global__ __launch_bounds__(V2_THREADS) void match_pipe_sim_kernel(const unsigned char* __restrict__ apk,
                                                                     const unsigned char* __restrict__ bpk,
                                                                     int R, int M, int G,
                                                                     float* __restrict__ sim,
                                                                     float* __restrict__ pval,      // [panels, R]
                                                                     int32_t* __restrict__ pidx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // PANEL_BYTES

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31;
    const int h = lane >> 5;
    const int g = blockIdx.x % G;
    const int panel = blockIdx.x / G;
    const int col0 = panel * PANEL_COLS;

    // panel fill and first operand load restated, as in match_pipe_kernel: this kernel's instructions are to stay as they are
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int gi = i * V2_THREADS + tid;
        const int col = gi >> 5, ch = gi & 31;
        const gdm_u32x4 v = *reinterpret_cast<const gdm_u32x4*>(bpk + (long)(col0 + col) * ROW_BYTES + ch * 16);
        *reinterpret_cast<gdm_u32x4*>(smem + gdm_swz<ROW_BYTES>(col, ch)) = v;
    }
    __syncthreads();

    const int nrb = R / V2_ROWS;
    if (g >= nrb) return;
    gdm_u32x4 areg[16];
    {
        const unsigned char* arow = apk + (long)(g * V2_ROWS + wave * 32 + lr) * ROW_BYTES;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            areg[s] = *reinterpret_cast<const gdm_u32x4*>(arow + (2 * s + h) * 16);
            areg[8 + s] = *reinterpret_cast<const gdm_u32x4*>(arow + (16 + 2 * s + h) * 16);
        }
    }
    float best[16];
    int bidx[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        best[i] = -INFINITY;
        bidx[i] = 0;
    }
    gdm_f32x16 a, b;
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = 0.f;
    BFrag1 fr = read_bfrag1(smem, lr, 0, h);
    const long Ml = M;
    const unsigned pvoff = (unsigned)(4 * h) * (unsigned)M + (unsigned)(col0 + lr);   // per-lane part of the store offset

    pipe_step_sim<0, 0, false, false>(smem, lr, h, areg, fr, a, b, best, bidx, 0, sim, 0u, Ml, apk);

    for (int rb = g; rb < nrb; rb += G) {
        const int row0 = rb * V2_ROWS + wave * 32;                        // uniform
        float* pbase = sim + (long)row0 * Ml;
        const bool has_next = rb + G < nrb;
        const int nrow = (has_next ? (rb + G) * V2_ROWS : rb * V2_ROWS) + wave * 32 + lr;
        const unsigned char* arow_next = apk + (long)nrow * ROW_BYTES;
        const int gc = col0 + lr;
        pipe_step_sim<1, 0, false, true>(smem, lr, h, areg, fr, b, a, best, bidx, gc, pbase, pvoff, Ml, arow_next);
        pipe_step_sim<2, 1, false, true>(smem, lr, h, areg, fr, a, b, best, bidx, gc + 32, pbase, pvoff, Ml, arow_next);
        pipe_step_sim<3, 2, false, true>(smem, lr, h, areg, fr, b, a, best, bidx, gc + 64, pbase, pvoff, Ml, arow_next);
        pipe_step_sim<4, 3, false, true>(smem, lr, h, areg, fr, a, b, best, bidx, gc + 96, pbase, pvoff, Ml, arow_next);
        pipe_step_sim<5, 4, false, true>(smem, lr, h, areg, fr, b, a, best, bidx, gc + 128, pbase, pvoff, Ml, arow_next);
        pipe_step_sim<6, 5, false, true>(smem, lr, h, areg, fr, a, b, best, bidx, gc + 160, pbase, pvoff, Ml, arow_next);
        pipe_step_sim<7, 6, true, true>(smem, lr, h, areg, fr, b, a, best, bidx, gc + 192, pbase, pvoff, Ml, arow_next);
        if (has_next) {
            pipe_step_sim<0, 7, false, true>(smem, lr, h, areg, fr, a, b, best, bidx, gc + 224, pbase, pvoff, Ml, arow_next);
        } else {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float v = b[reg];
                const bool t = v > best[reg];
                best[reg] = t ? v : best[reg];
                bidx[reg] = t ? gc + 224 : bidx[reg];
                float* o = pbase + (long)acc_row(0, reg, 0) * Ml + 224;
                __builtin_nontemporal_store(v, o + pvoff);
            }
        }
        finalize_rows(best, bidx, lane, h, row0, R, panel, pval, pidx);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            best[i] = -INFINITY;
            bidx[i] = 0;
        }
    }
}

// ------------------------------------------------------------------------------------------
// soft assignment: v2's panel kernel with log-sum-exp and expected-coordinate accumulation in the epilogue
// ------------------------------------------------------------------------------------------
// Per scene row i, over the M real columns j (include/gdm.h gdm_match_soft_packed_hip):
//   Z_i = sum_j exp(gamma (sim_ij - 1)),  S_i = sum_j exp(gamma (sim_ij - 1)) xyz_j;   lse = gamma + log Z, soft_xyz = S / Z.
// Cosines are <= 1 and gamma <= 40, so with the fixed shift 1 every term lies in [e^-80, ~1]: no running maximum, no rescaling, and
// the partial sums of the panels merge by addition.  The panel fill, the operand load, the product block (tile_product), the
// arg-max scan (running_max) and the row butterfly (finalize_rows) are match_panel_kernel's own, so best_idx / best_sim are the hard
// path's bit for bit (profiles/tile_helpers.md: what sharing them changed in either kernel's code, and that it cost no time).
// Layout as v2: lane = column, 16 rows per lane.  The four accumulators take 64 VGPRs per lane; they are paid for with v2's
// next-row-block operand prefetch (64 VGPRs), whose latency the SIMD's partner wave covers.  The panel's xyz (3 KiB) sits in LDS
// behind the descriptor panel.  Per row block a wave sums its 16 x 4 accumulators across the 32 lanes of each half-wave by the
// same halving butterfly as the arg-max (a fixed order: two launches are bit-identical) and writes one (Z, Sx, Sy, Sz) per
// (panel, row); soft_merge_kernel adds the panels in ascending order.  No atomics.
constexpr int SOFT_LDS_BYTES = PANEL_BYTES + PANEL_COLS * 3 * (int)sizeof(float);

// one halving step of the row butterfly for sums: the lane keeps the upper (up) or lower n of its 2n rows and adds the partner's
template <int n>
__device__ __forceinline__ void halve_sum(const float (&in)[2 * n], float (&out)[n], bool up, int mask)
{
    float ov[n];
#pragma unroll
    for (int i = 0; i < n; ++i) ov[i] = __shfl_xor(up ? in[i] : in[i + n], mask, 64);
    if constexpr (n == 8) GDM_SETTLE_LDS("+v"(ov[0]), "+v"(ov[1]), "+v"(ov[2]), "+v"(ov[3]), "+v"(ov[4]), "+v"(ov[5]), "+v"(ov[6]), "+v"(ov[7]));
    else if constexpr (n == 4) GDM_SETTLE_LDS("+v"(ov[0]), "+v"(ov[1]), "+v"(ov[2]), "+v"(ov[3]));
    else if constexpr (n == 2) GDM_SETTLE_LDS("+v"(ov[0]), "+v"(ov[1]));
    else GDM_SETTLE_LDS("+v"(ov[0]));
#pragma unroll
    for (int i = 0; i < n; ++i) out[i] = (up ? in[i + n] : in[i]) + ov[i];
}

// sum over the 32 lanes of a half-wave of each of the lane's 16 rows; lanes with (lane & 16) == 0 return row
// reg = 8*b0 + 4*b1 + 2*b2 + b3 of their lane bits (the row finalize_rows leaves there)
__device__ __forceinline__ float row_sum16(const float (&a)[16], int lane)
{
    float a8[8], a4[4], a2[2], a1[1];
    halve_sum<8>(a, a8, lane & 1, 1);
    halve_sum<4>(a8, a4, lane & 2, 2);
    halve_sum<2>(a4, a2, lane & 4, 4);
    halve_sum<1>(a2, a1, lane & 8, 8);
    float o = __shfl_xor(a1[0], 16, 64);
    GDM_SETTLE_LDS("+v"(o));
    return a1[0] + o;
}

template <int PREC>
__global__ __launch_bounds__(V2_THREADS) void match_panel_soft_kernel(const unsigned char* __restrict__ apk,
                                                                       const unsigned char* __restrict__ bpk,
                                                                       const float* __restrict__ xyz,     // [M, 3]
                                                                       int R, int M, int G, float k2,     // k2 = gamma log2(e)
                                                                       float* __restrict__ pval,          // [panels, R]
                                                                       int32_t* __restrict__ pidx,
                                                                       float4* __restrict__ psum)         // [panels, R] (Z, Sx, Sy, Sz)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // SOFT_LDS_BYTES
    float* xs = reinterpret_cast<float*>(smem + PANEL_BYTES);              // [PANEL_COLS][3]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lr = lane & 31;
    const int h = lane >> 5;
    const int g = blockIdx.x % G;
    const int panel = blockIdx.x / G;
    const int col0 = panel * PANEL_COLS;
    const int ncols = min(PANEL_COLS, M - col0);

    fill_panel(bpk, col0, M, tid);
    for (int i = tid; i < 3 * PANEL_COLS; i += V2_THREADS) {
        const int col = i / 3;
        xs[i] = xyz[(long)min(col0 + col, M - 1) * 3 + (i - 3 * col)];
    }
    __syncthreads();

    const int nrb = (R + V2_ROWS - 1) / V2_ROWS;
    for (int rb = g; rb < nrb; rb += G) {
        gdm_u32x4 areg[16];
        const int row0 = rb * V2_ROWS + wave * 32;
        load_a_rows<PREC>(apk, row0 + lr, R, h, areg);

        float best[16], z[16], sx[16], sy[16], sz[16];
        int bidx[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            best[i] = -INFINITY;
            bidx[i] = 0;
            z[i] = sx[i] = sy[i] = sz[i] = 0.f;
        }

#pragma unroll 1
        for (int cp = 0; cp < PANEL_COLS / 64; ++cp) {
            gdm_f32x16 acc[2];
            const int c0 = cp * 64 + lr, c1 = c0 + 32;
            tile_product<PREC, 2>(0, c0, h, areg, acc);
            const int gc0 = col0 + c0, gc1 = col0 + c1;
            const bool ok0 = c0 < ncols, ok1 = c1 < ncols;
            float x0 = xs[3 * c0], y0 = xs[3 * c0 + 1], z0 = xs[3 * c0 + 2];
            float x1 = xs[3 * c1], y1 = xs[3 * c1 + 1], z1 = xs[3 * c1 + 2];
            GDM_SETTLE_LDS("+v"(x0), "+v"(y0), "+v"(z0), "+v"(x1), "+v"(y1), "+v"(z1));
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float v0 = acc[0][reg], v1 = acc[1][reg];
                running_max(v0, gc0, ok0, best[reg], bidx[reg]);
                running_max(v1, gc1, ok1, best[reg], bidx[reg]);
                // a padding column of the last panel weighs nothing
                const float w0 = ok0 ? __builtin_amdgcn_exp2f(__builtin_fmaf(v0, k2, -k2)) : 0.f;
                const float w1 = ok1 ? __builtin_amdgcn_exp2f(__builtin_fmaf(v1, k2, -k2)) : 0.f;
                z[reg] = (z[reg] + w0) + w1;
                sx[reg] = __builtin_fmaf(w1, x1, __builtin_fmaf(w0, x0, sx[reg]));
                sy[reg] = __builtin_fmaf(w1, y1, __builtin_fmaf(w0, y0, sy[reg]));
                sz[reg] = __builtin_fmaf(w1, z1, __builtin_fmaf(w0, z0, sz[reg]));
            }
        }

        finalize_rows<true>(best, bidx, lane, h, row0, R, panel, pval, pidx);
        const float rz = row_sum16(z, lane), rx = row_sum16(sx, lane), ry = row_sum16(sy, lane), rw = row_sum16(sz, lane);
        if ((lane & 16) == 0) {
            const int grow = acc_row(row0, survivor_reg(lane), h);
            if (grow < R) psum[(long)panel * R + grow] = make_float4(rz, rx, ry, rw);
        }
    }
}

// panels in ascending order: (max, first arg-max) as merge_splits_kernel; Z and S by addition; then the three outputs, with the
// logarithm and the divisions in fp64 so that they add nothing to the error of the fp32 sums.  The numerator of conf is the best
// column's own term of Z, recomputed by the same two instructions from the same bits: every fp32 addition of non-negative terms
// is monotone, so Z >= that term (>= twice it when the column has an exact duplicate) and conf stays in (0, 1] (<= 0.5)
__global__ __launch_bounds__(256) void soft_merge_kernel(const float* __restrict__ pval, const int32_t* __restrict__ pidx,
                                                         const float4* __restrict__ psum, int panels, int R, float gamma, float k2,
                                                         float* __restrict__ oval, int32_t* __restrict__ oidx, float* __restrict__ lse,
                                                         float* __restrict__ conf, float* __restrict__ soft)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float v = pval[r];
    int ix = pidx[r];
    float4 s = psum[r];
    for (int p = 1; p < panels; ++p) {
        const float ov = pval[(long)p * R + r];
        if (ov > v) {
            v = ov;
            ix = pidx[(long)p * R + r];
        }
        const float4 o = psum[(long)p * R + r];
        s.x += o.x;
        s.y += o.y;
        s.z += o.z;
        s.w += o.w;
    }
    oval[r] = v;
    oidx[r] = ix;
    const double Z = (double)s.x, gm = (double)gamma;
    lse[r] = (float)(gm + log(Z));
    conf[r] = (float)((double)__builtin_amdgcn_exp2f(__builtin_fmaf(v, k2, -k2)) / Z);
    soft[3L * r] = (float)((double)s.y / Z);
    soft[3L * r + 1] = (float)((double)s.z / Z);
    soft[3L * r + 2] = (float)((double)s.w / Z);
}

__global__ __launch_bounds__(256) void merge_splits_kernel(const float* __restrict__ pval, const int32_t* __restrict__ pidx,
                                                           int splits, int R, float* __restrict__ oval, int32_t* __restrict__ oidx)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float v = pval[r];
    int ix = pidx[r];
    for (int s = 1; s < splits; ++s) {               // ascending column ranges: strict '>' keeps the first maximum
        const float ov = pval[(long)s * R + r];
        if (ov > v) {
            v = ov;
            ix = pidx[(long)s * R + r];
        }
    }
    oval[r] = v;
    oidx[r] = ix;
}

int pick_splits(int R, int M, bool write_sim)
{
    const int row_tiles = gdm_cdiv(R, MT_ROWS);
    const int max_splits = gdm_cdiv(M, MT_COLS);
    int want;
    if (write_sim) want = gdm_cdiv(M, 512);                 // ~512 columns per workgroup: thousands of workgroups
    else want = gdm_cdiv(1024, row_tiles);                  // >= ~4 workgroups per CU when the batch is small
    if (want < 1) want = 1;
    if (want > max_splits) want = max_splits;
    if (want > 64) want = 64;
    return want;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// 1 = tile-streaming kernel, 2 = LDS-resident panel kernel, 3 (default) = 2 + in-wave software pipeline where the shape allows;
// GDM_MATCH_KERNEL overrides, for A/B runs.
int match_kernel_version()
{
    const char* e = getenv("GDM_MATCH_KERNEL");
    if (e && e[0] == '1') return 1;
    if (e && e[0] == '2') return 2;
    return 3;
}

// score[b] = mean of conf over the points with mask != 0 (0 where there is none): one workgroup per crop, fp64, fixed order
__global__ __launch_bounds__(256) void match_score_kernel(const float* __restrict__ conf, const uint8_t* __restrict__ mask, int N,
                                                          float* __restrict__ score)
{
    __shared__ double red[4];
    __shared__ int cred[4];
    const int b = blockIdx.x;
    double s = 0.0;
    int c = 0;
    for (int i = threadIdx.x; i < N; i += 256) {
        if (!mask[(long)b * N + i]) continue;
        s += (double)conf[(long)b * N + i];
        c += 1;
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = s;
        cred[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = cred[0] + cred[1] + cred[2] + cred[3];
        score[b] = n > 0 ? (float)(((red[0] + red[1]) + (red[2] + red[3])) / (double)n) : 0.f;
    }
}

// ------------------------------------------------------------------------------------------
// two-way matching: v2's panel kernel with the masked column arg-max of every crop taken from the same accumulators
// ------------------------------------------------------------------------------------------
// include/gdm.h THE TWO-WAY RULE.  The panel fill, the operand load, the product block, the row scan and the row butterfly are
// match_panel_kernel's own (best_idx / best_sim are the hard path's bit for bit); like the soft kernel this one gives up v2's operand
// prefetch.  The reverse direction, per 64-column step and per crop c that the wave's 32 rows touch (one, or two at a crop boundary;
// more only when N < 32):
//   1. in-lane: a scan of the lane's 16 registers (ascending rows, strict '>': the lowest row on ties) under the bits of the rows
//      that are masked and belong to c;
//   2. the two half-waves by one shuffle (rows interleave in fours, so the row decides ties);
//   3. the 8 waves: a 64-bit unsigned atomic maximum of the key into the workgroup's column buffer in LDS, one slot of 256 keys per
//      crop of the row block (the compiler folds this and the direct form of step 4 into one flat_atomic_umax_x2);
//   4. the row blocks (and the crops past the TW_SLOTS a row block has slots for, which skip step 3): global_atomic_umax_x2 of the
//      key into keys[crop][column], from the buffer after a barrier, 2 KiB contiguous per slot.
// key = order-preserving image of the similarity << 32 | ~(row in the crop): an integer maximum picks the larger similarity, then the
// lower row, whatever the arrival order; 0 (below every real key) means no candidate.  twoway_cols_kernel decodes.
constexpr int TW_SLOTS = 2;                             // crops of one row block that merge in LDS: all of them when N >= 255
constexpr int TWOWAY_LDS_BYTES = PANEL_BYTES + TW_SLOTS * PANEL_COLS * (int)sizeof(unsigned long long);

__device__ __forceinline__ unsigned long long col_key(float v, int row)
{
    unsigned u = __float_as_uint(v + 0.f);              // -0 -> +0: the two compare equal and must share a key
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned)~row;
}

// bit reg is set iff row acc_row(0, reg, 0) of the lane is masked (mbits) and lies in [lo, lo + n)
__device__ __forceinline__ unsigned crop_rows(unsigned mbits, int lo, int n)
{
    unsigned b = 0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) b |= (unsigned)(acc_row(0, reg, 0) - lo) < (unsigned)n ? 1u << reg : 0u;
    return b & mbits;
}

// steps 1 to 3 (or 4) for one column of the lane: a = its 16 similarities, bits = the rows that count, rbase = the row in the crop
// of the lane's register 0; the key goes to lds (the column's key in the workgroup's buffer) if in_lds, else to gkey directly
__device__ __forceinline__ void col_reduce(const gdm_f32x16& a, unsigned bits, int rbase, bool ok, int h, bool in_lds,
                                           unsigned long long* lds, unsigned long long* gkey)
{
    float bv = -INFINITY;
    int row = -1;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) running_max(a[reg], rbase + acc_row(0, reg, 0), (bits >> reg) & 1u, bv, row);
    const float ov = __shfl_xor(bv, 32, 64);
    const int orow = __shfl_xor(row, 32, 64);
    if (ov > bv || (ov == bv && (unsigned)orow < (unsigned)row)) {      // no candidate is row -1: the largest unsigned
        bv = ov;
        row = orow;
    }
    if (h == 0 && ok && row >= 0) {
        const unsigned long long key = col_key(bv, row);
        if (in_lds) atomicMax(lds, key);
        else atomicMax(gkey, key);
    }
}

// col_reduce's steps 2 and 3 alone, for the dual kernel, which takes step 1 inside its own loop over the registers (its accumulators
// do not outlive that loop): (bv, row) = what step 1 left in the lane, row -1 where no row counted; the key goes to lds.  The same
// comparisons and the same key: written twice so that col_reduce, and with it the two-way kernel's code, stays as it was
__device__ __forceinline__ void col_merge(float bv, int row, bool ok, int h, unsigned long long* lds)
{
    const float ov = __shfl_xor(bv, 32, 64);
    const int orow = __shfl_xor(row, 32, 64);
    if (ov > bv || (ov == bv && (unsigned)orow < (unsigned)row)) {
        bv = ov;
        row = orow;
    }
    if (h == 0 && ok && row >= 0) atomicMax(lds, col_key(bv, row));
}

template <int PREC>
__global__ __launch_bounds__(V2_THREADS) void match_panel_twoway_kernel(const unsigned char* __restrict__ apk,
                                                                         const unsigned char* __restrict__ bpk,
                                                                         const uint8_t* __restrict__ mask,       // [R]
                                                                         int R, int N, int M, int G,
                                                                         float* __restrict__ pval,               // [panels, R]
                                                                         int32_t* __restrict__ pidx,
                                                                         unsigned long long* __restrict__ keys)  // [R / N, M]
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // TWOWAY_LDS_BYTES
    unsigned long long* cbuf = reinterpret_cast<unsigned long long*>(smem + PANEL_BYTES);   // [TW_SLOTS][PANEL_COLS]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lr = lane & 31;
    const int h = lane >> 5;
    const int g = blockIdx.x % G;
    const int panel = blockIdx.x / G;
    const int col0 = panel * PANEL_COLS;
    const int ncols = min(PANEL_COLS, M - col0);

    fill_panel(bpk, col0, M, tid);
    static_assert(TW_SLOTS * PANEL_COLS == V2_THREADS, "one key of the column buffer per thread");
    cbuf[tid] = 0ull;
    __syncthreads();

    const int nrb = (R + V2_ROWS - 1) / V2_ROWS;
    for (int rb = g; rb < nrb; rb += G) {
        gdm_u32x4 areg[16];
        const int row0 = rb * V2_ROWS + wave * 32;
        load_a_rows<PREC>(apk, row0 + lr, R, h, areg);

        // the lane's 16 rows: which are real and masked; the crops the wave's rows touch, and the first crop of the row block
        unsigned mbits = 0;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int grow = acc_row(row0, reg, h);
            if (grow < R && mask[grow]) mbits |= 1u << reg;
        }
        const int lrow0 = row0 + 4 * h;                                    // the lane's register 0
        const int cfirst = (rb * V2_ROWS) / N;
        const int cb0 = row0 / N;
        const int cb1 = row0 < R ? min(row0 + 31, R - 1) / N : cb0 - 1;     // a wave past the last row has no crop
        const unsigned bits0 = crop_rows(mbits, cb0 * N - lrow0, N);

        float best[16];
        int bidx[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            best[i] = -INFINITY;
            bidx[i] = 0;
        }

#pragma unroll 1
        for (int cp = 0; cp < PANEL_COLS / 64; ++cp) {
            gdm_f32x16 acc[2];
            const int c0 = cp * 64 + lr, c1 = c0 + 32;
            tile_product<PREC, 2>(0, c0, h, areg, acc);
            const int gc0 = col0 + c0, gc1 = col0 + c1;
            const bool ok0 = c0 < ncols, ok1 = c1 < ncols;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                running_max(acc[0][reg], gc0, ok0, best[reg], bidx[reg]);
                running_max(acc[1][reg], gc1, ok1, best[reg], bidx[reg]);
            }
#pragma unroll 1
            for (int c = cb0; c <= cb1; ++c) {
                const int rbase = lrow0 - c * N;
                const unsigned bits = c == cb0 ? bits0 : crop_rows(mbits, -rbase, N);
                const bool in_lds = c - cfirst < TW_SLOTS;
                unsigned long long* slot = cbuf + (in_lds ? c - cfirst : 0) * PANEL_COLS;
                unsigned long long* gk = keys + (long)c * M + col0;
                col_reduce(acc[0], bits, rbase, ok0, h, in_lds, slot + c0, gk + c0);
                col_reduce(acc[1], bits, rbase, ok1, h, in_lds, slot + c1, gk + c1);
            }
        }

        finalize_rows<true>(best, bidx, lane, h, row0, R, panel, pval, pidx);

        // step 4: the row block's keys leave the buffer (one thread per key) and the buffer is empty again for the next row block
        __syncthreads();
        {
            const int c = cfirst + tid / PANEL_COLS, col = tid % PANEL_COLS;
            const unsigned long long key = cbuf[tid];
            if (key != 0ull) {                                             // only columns < ncols of crops < R / N were ever written
                atomicMax(keys + (long)c * M + col0 + col, key);
                cbuf[tid] = 0ull;
            }
        }
        __syncthreads();
    }
}

// key -> (col_idx, col_sim); 0 -> (-1, -inf)
__global__ __launch_bounds__(256) void twoway_cols_kernel(const unsigned long long* __restrict__ keys, long n, int32_t* __restrict__ col_idx,
                                                          float* __restrict__ col_sim)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    const unsigned u = (unsigned)(key >> 32);
    col_idx[i] = key ? (int32_t)~(unsigned)key : -1;
    col_sim[i] = key ? __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u) : -INFINITY;
}

// include/gdm.h THE CYCLE RULE: one workgroup per crop, one pass over its points, an integer count
__global__ __launch_bounds__(256) void match_cycle_kernel(const float* __restrict__ scene_xyz, long scene_bstride, int pt_stride, int ch_stride,
                                                          const int32_t* __restrict__ best_idx, const int32_t* __restrict__ col_idx,
                                                          const uint8_t* __restrict__ mask, int N, int M, float r2,
                                                          uint8_t* __restrict__ pair_mask, int32_t* __restrict__ pair_count,
                                                          float* __restrict__ cycle_d2)
{
    __shared__ int cred[4];
    const int b = blockIdx.x;
    const float* sp = scene_xyz + (long)b * scene_bstride;
    int c = 0;
    for (int i = threadIdx.x; i < N; i += 256) {
        float d2 = INFINITY;
        bool keep = false;
        if (mask[(long)b * N + i]) {
            const int j = best_idx[(long)b * N + i];
            const int k = (j >= 0 && j < M) ? col_idx[(long)b * M + j] : -1;
            if (k >= 0 && k < N) {
                const float* pi = sp + (long)i * pt_stride;
                const float* pk = sp + (long)k * pt_stride;
                const float dx = __fsub_rn(pi[0], pk[0]);
                const float dy = __fsub_rn(pi[ch_stride], pk[ch_stride]);
                const float dz = __fsub_rn(pi[2L * ch_stride], pk[2L * ch_stride]);
                d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                keep = d2 <= r2;                                           // false for a NaN
            }
        }
        pair_mask[(long)b * N + i] = keep ? 1 : 0;
        cycle_d2[(long)b * N + i] = d2;
        c += keep ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) pair_count[b] = cred[0] + cred[1] + cred[2] + cred[3];
}

// ------------------------------------------------------------------------------------------
// dual-softmax matching: the soft kernel's row softmax, the two-way kernel's column arg-max and the column sum of the soft weights
// ------------------------------------------------------------------------------------------
// include/gdm.h THE DUAL RULE.  One pass of MFMAs gives all three.  The panel fill, the operand load, the product block, the row scan,
// the row butterflies (finalize_rows, row_sum16) and the weight w = exp2(fma(sim, k2, -k2)) are match_panel_soft_kernel's own, the
// column key scan (col_reduce's comparisons and key) is match_panel_twoway_kernel's: the row outputs are the soft launch's bit for bit and col_idx /
// col_sim the two-way launch's.  Unlike those two kernels this one cuts the rows into blocks that never span a crop: ceil(N / 256)
// blocks of 256 rows per crop, the rows past the crop's end unreal (loaded clamped, never written, never counted).  One crop per row
// block means one key slot and one sum slot in LDS and no crop loop.  The helpers are addressed crop by crop: the crop's rows as a
// launch of N rows, the partials through pointers moved so that finalize_rows' [panel * N + row] lands on [panel * R + c * N + row].
// A step is ONE 32-column accumulator block (tile_product<PREC, 1>), where those kernels take two: 16 accumulator VGPRs less, which
// is what lets all three results fit in 256 VGPRs without scratch (241 / 249, profiles/match_dual.md).  z + w and fma(w, x, s) run
// over the same columns in the same order as the soft kernel's (z + w0) + w1 and nested fmas: the same bits.
// The column sum, per step and for the lane's column, reuses the w of the row sums (no further exponential):
//   1. in-lane: the lane's 16 rows in ascending register order, under the bits of the rows that are real and masked;
//   2. the other half-wave by one shuffle (a + b = b + a: both halves hold the same bits);
//   3. the 8 waves: each writes its partial to wsum[wave][column] in LDS (every wave writes every column of every row block, so the
//      buffer needs no reset); after the barrier the key flush has anyway one thread per column adds them in ascending wave order
//      and writes cpart[row block][column];
//   4. the row blocks of a crop: dual_cols_kernel adds them in ascending order.
// A fixed order throughout and no floating-point atomic: two launches give the same bytes.
constexpr int DUAL_KEY_OFF = SOFT_LDS_BYTES;                                            // [PANEL_COLS] keys of the row block's crop
constexpr int DUAL_SUM_OFF = DUAL_KEY_OFF + PANEL_COLS * (int)sizeof(unsigned long long);   // [8 waves][PANEL_COLS] column sums
constexpr int DUAL_LDS_BYTES = DUAL_SUM_OFF + (V2_THREADS / 64) * PANEL_COLS * (int)sizeof(float);
static_assert(DUAL_KEY_OFF % 8 == 0 && DUAL_LDS_BYTES <= 160 * 1024, "the dual kernel's LDS: 128 KiB panel + 3 KiB xyz + 2 KiB keys + 8 KiB sums");

template <int PREC>
__global__ __launch_bounds__(V2_THREADS) void match_panel_dual_kernel(const unsigned char* __restrict__ apk,
                                                                       const unsigned char* __restrict__ bpk,
                                                                       const float* __restrict__ xyz,          // [M, 3]
                                                                       const uint8_t* __restrict__ mask,       // [B, N]
                                                                       int B, int N, int M, int G, float k2,
                                                                       float* __restrict__ pval,               // [panels, R]
                                                                       int32_t* __restrict__ pidx,
                                                                       float4* __restrict__ psum,              // [panels, R]
                                                                       unsigned long long* __restrict__ keys,  // [B, M]
                                                                       float* __restrict__ cpart)              // [B * nrbc, M]
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // DUAL_LDS_BYTES
    float* xs = reinterpret_cast<float*>(smem + PANEL_BYTES);              // [PANEL_COLS][3]
    unsigned long long* cbuf = reinterpret_cast<unsigned long long*>(smem + DUAL_KEY_OFF);
    float* wsum = reinterpret_cast<float*>(smem + DUAL_SUM_OFF);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);         // uniform: what derives from it stays out of the VGPRs
    const int lr = lane & 31;
    const int h = lane >> 5;
    const int g = blockIdx.x % G;
    const int panel = blockIdx.x / G;
    const int col0 = panel * PANEL_COLS;
    const int ncols = min(PANEL_COLS, M - col0);
    const int R = B * N;

    fill_panel(bpk, col0, M, tid);
    for (int i = tid; i < 3 * PANEL_COLS; i += V2_THREADS) {
        const int col = i / 3;
        xs[i] = xyz[(long)min(col0 + col, M - 1) * 3 + (i - 3 * col)];
    }
    if (tid < PANEL_COLS) cbuf[tid] = 0ull;
    __syncthreads();

    const int nrbc = (N + V2_ROWS - 1) / V2_ROWS;                          // row blocks per crop
    const int nq = B * nrbc;
    for (int q = g; q < nq; q += G) {
        gdm_u32x4 areg[16];
        const int c = q / nrbc;
        const long crow = (long)c * N;                                     // the crop's first row
        const int row0 = (q - c * nrbc) * V2_ROWS + wave * 32;             // counted inside the crop
        load_a_rows<PREC>(apk + crow * ROW_BYTES, row0 + lr, N, h, areg);

        unsigned mbits = 0;                                                // the lane's 16 rows: which are real and masked
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int lrow = acc_row(row0, reg, h);
            if (lrow < N && mask[crow + lrow]) mbits |= 1u << reg;
        }

        float best[16], z[16], sx[16], sy[16], sz[16];
        int bidx[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            best[i] = -INFINITY;
            bidx[i] = 0;
            z[i] = sx[i] = sy[i] = sz[i] = 0.f;
        }

#pragma unroll 1
        for (int cb = 0; cb < PANEL_COLS / 32; ++cb) {
            gdm_f32x16 acc[1];
            const int c0 = cb * 32 + lr;
            tile_product<PREC, 1>(0, c0, h, areg, acc);
            // the step's column bookkeeping is formed from the lane behind the products, step by step, not held across them (the
            // tail below says why)
            int lc = lane;
            asm volatile("" : "+v"(lc));
            const int cc = cb * 32 + (lc & 31), hc = lc >> 5;              // = c0, h
            const int gc0 = col0 + cc;
            const bool ok0 = cc < ncols;
            float x0 = xs[3 * cc], y0 = xs[3 * cc + 1], z0 = xs[3 * cc + 2];
            GDM_SETTLE_LDS("+v"(x0), "+v"(y0), "+v"(z0));
            float cs0 = 0.f, kv0 = -INFINITY;
            int kr0 = -1;
            const int krow = row0 + 4 * hc;                                // the lane's register 0, counted inside the crop
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float v0 = acc[0][reg];
                running_max(v0, gc0, ok0, best[reg], bidx[reg]);
                // a padding column of the last panel weighs nothing
                const float w0 = ok0 ? __builtin_amdgcn_exp2f(__builtin_fmaf(v0, k2, -k2)) : 0.f;
                z[reg] = z[reg] + w0;
                sx[reg] = __builtin_fmaf(w0, x0, sx[reg]);
                sy[reg] = __builtin_fmaf(w0, y0, sy[reg]);
                sz[reg] = __builtin_fmaf(w0, z0, sz[reg]);
                const bool on = (mbits >> reg) & 1u;                       // step 1 of the column sum and of the column arg-max
                cs0 += on ? w0 : 0.f;
                running_max(v0, krow + acc_row(0, reg, 0), on, kv0, kr0);
            }
            cs0 += __shfl_xor(cs0, 32, 64);                                // step 2
            if (hc == 0) wsum[wave * PANEL_COLS + cc] = cs0;               // step 3: this wave's partial of the row block
            col_merge(kv0, kr0, ok0, hc, cbuf + cc);
        }

        // what the tail derives from the lane is formed here, row block by row block: hoisted out of the loop it would sit in
        // registers through the products, which have none to spare
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int hn = ln >> 5;
        const long poff = crow + (long)panel * (R - N);                    // [panel * N + row] from here = [panel * R + crow + row]
        finalize_rows<true>(best, bidx, ln, hn, row0, N, panel, pval + poff, pidx + poff);
        const float rz = row_sum16(z, ln), rx = row_sum16(sx, ln), ry = row_sum16(sy, ln), rw = row_sum16(sz, ln);
        if ((ln & 16) == 0) {
            const int lrow = acc_row(row0, survivor_reg(ln), hn);
            if (lrow < N) psum[(long)panel * R + crow + lrow] = make_float4(rz, rx, ry, rw);
        }

        // the row block's keys and sums leave LDS, one thread per column; the key buffer is empty again for the next row block
        __syncthreads();
        const int col = wave * 64 + ln;
        if (col < PANEL_COLS) {
            const unsigned long long key = cbuf[col];
            if (key != 0ull) {                                             // only columns < ncols were ever written
                atomicMax(keys + (long)c * M + col0 + col, key);
                cbuf[col] = 0ull;
            }
            if (col < ncols) {
                float s = wsum[col];
#pragma unroll
                for (int w = 1; w < V2_THREADS / 64; ++w) s += wsum[w * PANEL_COLS + col];      // ascending waves
                cpart[(long)q * M + col0 + col] = s;
            }
        }
        __syncthreads();
    }
}

// per (crop, vertex): Zc = the row blocks' partials in ascending order; the key decoded as twoway_cols_kernel does it; col_lse with
// the logarithm in fp64 as soft_merge_kernel; col_conf = the w of col_sim, recomputed by the same two instructions, over Zc.  That w is
// one of Zc's terms and fp32 addition of non-negative terms is monotone, so col_conf lies in (0, 1].
__global__ __launch_bounds__(256) void dual_cols_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ cpart, long n,
                                                        int nrbc, int M, float gamma, float k2, int32_t* __restrict__ col_idx,
                                                        float* __restrict__ col_sim, float* __restrict__ col_lse, float* __restrict__ col_conf,
                                                        float* __restrict__ zc)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long b = i / M;
    const int j = (int)(i - b * M);
    const float* p = cpart + b * nrbc * M + j;
    float s = p[0];
    for (int k = 1; k < nrbc; ++k) s += p[(long)k * M];
    const unsigned long long key = keys[i];
    const unsigned u = (unsigned)(key >> 32);
    const float sim = key ? __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u) : -INFINITY;
    col_idx[i] = key ? (int32_t)~(unsigned)key : -1;
    col_sim[i] = sim;
    zc[i] = s;
    col_lse[i] = (float)((double)gamma + log((double)s));                  // log 0 = -inf: a crop with no masked point
    col_conf[i] = key ? (float)((double)__builtin_amdgcn_exp2f(__builtin_fmaf(sim, k2, -k2)) / (double)s) : 0.f;
}

// dual[i] = conf[i] * (w_ij / Zc[b, j]) at j = best_idx[i] for a masked point, the quotient and the product in fp64 and one rounding;
// 0 for an unmasked point.  The point is one of Zc's terms, so the quotient is <= 1 and dual <= conf.
__global__ __launch_bounds__(256) void dual_rows_kernel(const int32_t* __restrict__ best_idx, const float* __restrict__ best_sim,
                                                        const float* __restrict__ conf, const uint8_t* __restrict__ mask,
                                                        const float* __restrict__ zc, int R, int N, int M, float k2, float* __restrict__ dual)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float d = 0.f;
    if (mask[r]) {
        const int j = min(max(best_idx[r], 0), M - 1);
        const double w = (double)__builtin_amdgcn_exp2f(__builtin_fmaf(best_sim[r], k2, -k2));
        d = (float)((double)conf[r] * (w / (double)zc[(long)(r / N) * M + j]));
    }
    dual[r] = d;
}

} // namespace

extern "C" size_t gdm_match_rows_bytes(int rows)
{
    return rows < 1 ? 0 : align256((size_t)rows * ROW_BYTES);
}

extern "C" size_t gdm_match_partial_bytes(int B, int N)
{
    if (B < 1 || N < 1) return 0;
    return 2 * align256(64 * (size_t)B * N * sizeof(float));
}

extern "C" size_t gdm_match_workspace_bytes(int B, int N, int M)
{
    if (B < 1 || N < 1 || M < 1) return 0;
    return gdm_match_rows_bytes(B * N) + gdm_match_rows_bytes(M) + gdm_match_partial_bytes(B, N) + 256;
}

extern "C" int gdm_match_pack_hip(const float* x, int R, int Dd, int n, int precision, void* rows, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    GDM_CHECK_ARG(x && rows, "gdm_match_pack_hip: NULL pointer");
    GDM_CHECK_ARG(Dd == D, "gdm_match_pack_hip: D=%d, only D=128 is built", Dd);
    GDM_CHECK_ARG(R >= 1 && R <= 65535 && n >= 1, "gdm_match_pack_hip: bad shape R=%d n=%d", R, n);
    GDM_CHECK_ARG(precision == GDM_MATCH_BF16X3 || precision == GDM_MATCH_F32, "gdm_match_pack_hip: precision=%d", precision);
    GDM_CHECK_ARG(((uintptr_t)rows & 15) == 0, "gdm_match_pack_hip: rows must be 16-byte aligned");
    dim3 grid(gdm_cdiv(n, 64), R);
    if (precision == GDM_MATCH_BF16X3)
        hipLaunchKernelGGL(pack_rows_kernel<GDM_MATCH_BF16X3>, grid, dim3(256), 0, stream, x, n, (unsigned char*)rows);
    else
        hipLaunchKernelGGL(pack_rows_kernel<GDM_MATCH_F32>, grid, dim3(256), 0, stream, x, n, (unsigned char*)rows);
    return gdm_launch_status("pack_rows_kernel");
}

extern "C" int gdm_match_pack2_hip(const float* x1, int R1, int n1, void* rows1, const float* x2, int R2, int n2, void* rows2,
                                   int Dd, int precision, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    GDM_CHECK_ARG(x1 && rows1 && x2 && rows2, "gdm_match_pack2_hip: NULL pointer");
    GDM_CHECK_ARG(Dd == D, "gdm_match_pack2_hip: D=%d, only D=128 is built", Dd);
    GDM_CHECK_ARG(R1 >= 1 && R2 >= 1 && R1 + R2 <= 65535 && n1 >= 1 && n2 >= 1, "gdm_match_pack2_hip: bad shape R=%d+%d n=%d,%d", R1, R2, n1, n2);
    GDM_CHECK_ARG(precision == GDM_MATCH_BF16X3 || precision == GDM_MATCH_F32, "gdm_match_pack2_hip: precision=%d", precision);
    GDM_CHECK_ARG((((uintptr_t)rows1 | (uintptr_t)rows2) & 15) == 0, "gdm_match_pack2_hip: rows must be 16-byte aligned");
    dim3 grid(gdm_cdiv(n1 > n2 ? n1 : n2, 64), R1 + R2);
    if (precision == GDM_MATCH_BF16X3)
        hipLaunchKernelGGL(pack_rows2_kernel<GDM_MATCH_BF16X3>, grid, dim3(256), 0, stream, x1, R1, n1, (unsigned char*)rows1, x2, n2, (unsigned char*)rows2);
    else
        hipLaunchKernelGGL(pack_rows2_kernel<GDM_MATCH_F32>, grid, dim3(256), 0, stream, x1, R1, n1, (unsigned char*)rows1, x2, n2, (unsigned char*)rows2);
    return gdm_launch_status("pack_rows2_kernel");
}

extern "C" int gdm_match_packed_hip(const void* scene_rows, const void* model_rows, int R, int M, int precision,
                                    int32_t* best_idx, float* best_sim, float* sim,
                                    void* partial, size_t partial_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    GDM_CHECK_ARG(scene_rows && model_rows && best_idx && best_sim && partial, "gdm_match_packed_hip: NULL pointer");
    GDM_CHECK_ARG(R >= 1 && M >= 1, "gdm_match_packed_hip: bad shape R=%d M=%d", R, M);
    GDM_CHECK_ARG(precision == GDM_MATCH_BF16X3 || precision == GDM_MATCH_F32, "gdm_match_packed_hip: precision=%d", precision);
    GDM_CHECK_ARG((((uintptr_t)scene_rows | (uintptr_t)model_rows) & 15) == 0, "gdm_match_packed_hip: the packed rows must be 16-byte aligned");
    const size_t half = align256(64 * (size_t)R * sizeof(float));
    if (partial_bytes < 2 * half) {
        gdm_set_error("gdm_match_packed_hip: partial workspace %zu < %zu bytes", partial_bytes, 2 * half);
        return GDM_ENOMEM;
    }
    const unsigned char* apk = (const unsigned char*)scene_rows;
    const unsigned char* bpk = (const unsigned char*)model_rows;
    float* pval = (float*)partial;
    int32_t* pidx = (int32_t*)((unsigned char*)partial + half);

    const bool ws_sim = sim != nullptr;
    int rc;
    const int panels = gdm_cdiv(M, PANEL_COLS);
    int nsplit;
    const int mkv = match_kernel_version();
    if (mkv >= 2 && panels <= 64) {
        // ---- v2: LDS-resident model panel, one persistent-ish workgroup per (panel, row group) ----
        const int nrb = gdm_cdiv(R, V2_ROWS);
        const bool pipe = mkv == 3 && precision == GDM_MATCH_BF16X3 && R % V2_ROWS == 0 && M % PANEL_COLS == 0 &&
                          (long)R * M < (1L << 40) && (long)32 * M < (1L << 30);
        // one workgroup per CU (the panel takes the LDS): v2 queues two rounds; v3 runs one round of <= 256 workgroups,
        // which the store path prefers (tools/micro/store_pattern.hip: 5.9 vs 4.9 TB/s)
        int G = (pipe ? 256 : 512) / panels;
        if (G < 1) G = 1;
        if (G > nrb) G = nrb;
        if (G >= 8) G &= ~7;                                    // keep same-rows workgroups on one bid%8 class
        nsplit = panels;
        dim3 grid(panels * G);
        float* ov = nsplit == 1 ? best_sim : pval;
        int32_t* oi = nsplit == 1 ? best_idx : pidx;
        static_assert(GDM_MATCH_BF16X3 == 0 && GDM_MATCH_F32 == 1, "the precision is dispatched as an index");
        gdm_dispatch_bool(ws_sim, [&](auto WS) {
            gdm_dispatch_int<3>(pipe ? 2 : precision, [&](auto K) {            // the panel kernel at either precision, or the pipelined pair
                constexpr bool W = decltype(WS)::value;
                constexpr int k = decltype(K)::value;
                constexpr auto kernel = k < 2 ? match_panel_kernel<k & 1, W> : W ? match_pipe_sim_kernel : match_pipe_kernel;
                gdm_allow_lds<kernel>(PANEL_BYTES);
                hipLaunchKernelGGL(kernel, grid, dim3(V2_THREADS), PANEL_BYTES, stream, apk, bpk, R, M, G, sim, ov, oi);
            });
        });
        rc = gdm_launch_status("match_panel_kernel");
        if (rc) return rc;
    } else {
        const int splits = pick_splits(R, M, ws_sim);
        int cps = gdm_cdiv(gdm_cdiv(M, splits), MT_COLS) * MT_COLS;
        nsplit = gdm_cdiv(M, cps);
        dim3 grid(gdm_cdiv(R, MT_ROWS), nsplit);
        float* ov = nsplit == 1 ? best_sim : pval;
        int32_t* oi = nsplit == 1 ? best_idx : pidx;
        const size_t lds = 2 * TILE_BYTES;
        gdm_dispatch_int<2>(precision, [&](auto P) {                // GDM_MATCH_BF16X3 = 0, GDM_MATCH_F32 = 1 (asserted above)
            gdm_dispatch_bool(ws_sim, [&](auto WS) {
                hipLaunchKernelGGL((match_kernel<decltype(P)::value, decltype(WS)::value>), grid, dim3(256), lds, stream, apk, bpk, R, M, cps, sim, ov, oi);
            });
        });
        rc = gdm_launch_status("match_kernel");
        if (rc) return rc;
    }
    if (nsplit > 1) {
        hipLaunchKernelGGL(merge_splits_kernel, dim3(gdm_cdiv(R, 256)), dim3(256), 0, stream, pval, pidx, nsplit, R, best_sim, best_idx);
        rc = gdm_launch_status("merge_splits_kernel");
    }
    return rc;
}

extern "C" size_t gdm_match_soft_partial_bytes(int B, int N)
{
    if (B < 1 || N < 1) return 0;
    return gdm_match_partial_bytes(B, N) + align256(64 * (size_t)B * N * sizeof(float4));
}

extern "C" int gdm_match_soft_packed_hip(const void* scene_rows, const void* model_rows, const float* model_xyz, int R, int M,
                                         int precision, float gamma, int32_t* best_idx, float* best_sim, float* lse, float* conf,
                                         float* soft_xyz, void* partial, size_t partial_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    GDM_CHECK_ARG(scene_rows && model_rows && model_xyz && best_idx && best_sim && lse && conf && soft_xyz && partial,
                  "gdm_match_soft_packed_hip: NULL pointer");
    GDM_CHECK_ARG(R >= 1 && M >= 1, "gdm_match_soft_packed_hip: bad shape R=%d M=%d", R, M);
    GDM_CHECK_ARG(M <= GDM_MATCH_SOFT_MAX_M, "gdm_match_soft_packed_hip: M=%d, the soft kernel covers M <= %d", M, GDM_MATCH_SOFT_MAX_M);
    GDM_CHECK_ARG(precision == GDM_MATCH_BF16X3 || precision == GDM_MATCH_F32, "gdm_match_soft_packed_hip: precision=%d", precision);
    GDM_CHECK_ARG(gamma > 0.f && gamma <= GDM_MATCH_SOFT_MAX_GAMMA, "gdm_match_soft_packed_hip: gamma=%g not in (0, %g]", (double)gamma,
                  (double)GDM_MATCH_SOFT_MAX_GAMMA);                       // a NaN fails both comparisons
    GDM_CHECK_ARG(((uintptr_t)partial & 15) == 0, "gdm_match_soft_packed_hip: partial must be 16-byte aligned");
    GDM_CHECK_ARG((((uintptr_t)scene_rows | (uintptr_t)model_rows) & 15) == 0, "gdm_match_soft_packed_hip: the packed rows must be 16-byte aligned");
    const size_t half = align256(64 * (size_t)R * sizeof(float));
    const size_t need = 2 * half + align256(64 * (size_t)R * sizeof(float4));
    if (partial_bytes < need) {
        gdm_set_error("gdm_match_soft_packed_hip: partial workspace %zu < %zu bytes", partial_bytes, need);
        return GDM_ENOMEM;
    }
    static_assert(GDM_MATCH_SOFT_MAX_M == 64 * PANEL_COLS, "the partial workspace holds 64 panels");
    float* pval = (float*)partial;
    int32_t* pidx = (int32_t*)((unsigned char*)partial + half);
    float4* psum = (float4*)((unsigned char*)partial + 2 * half);
    const int panels = gdm_cdiv(M, PANEL_COLS);
    const int nrb = gdm_cdiv(R, V2_ROWS);
    int G = 512 / panels;                                       // as v2: one workgroup per CU, two rounds
    if (G < 1) G = 1;
    if (G > nrb) G = nrb;
    if (G >= 8) G &= ~7;
    const float k2 = gamma * 1.44269504088896340736f;
    gdm_dispatch_int<2>(precision, [&](auto P) {
        constexpr auto kernel = match_panel_soft_kernel<decltype(P)::value>;
        gdm_allow_lds<kernel>(SOFT_LDS_BYTES);
        hipLaunchKernelGGL(kernel, dim3(panels * G), dim3(V2_THREADS), SOFT_LDS_BYTES, stream, (const unsigned char*)scene_rows,
                           (const unsigned char*)model_rows, model_xyz, R, M, G, k2, pval, pidx, psum);
    });
    int rc = gdm_launch_status("match_panel_soft_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(soft_merge_kernel, dim3(gdm_cdiv(R, 256)), dim3(256), 0, stream, pval, pidx, psum, panels, R, gamma, k2, best_sim,
                       best_idx, lse, conf, soft_xyz);
    return gdm_launch_status("soft_merge_kernel");
}

extern "C" int gdm_match_score_hip(const float* conf, const uint8_t* mask, int B, int N, float* score, void* stream)
{
    GDM_CHECK_ARG(conf && mask && score, "gdm_match_score_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && N >= 1, "gdm_match_score_hip: bad shape B=%d N=%d", B, N);
    hipLaunchKernelGGL(match_score_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, conf, mask, N, score);
    return gdm_launch_status("match_score_kernel");
}

extern "C" size_t gdm_match_twoway_partial_bytes(int B, int N, int M)
{
    if (B < 1 || N < 1 || M < 1) return 0;
    return gdm_match_partial_bytes(B, N) + align256((size_t)B * M * sizeof(unsigned long long));
}

extern "C" int gdm_match_twoway_packed_hip(const void* scene_rows, const void* model_rows, const uint8_t* mask, int B, int N, int M,
                                           int precision, int32_t* best_idx, float* best_sim, int32_t* col_idx, float* col_sim,
                                           void* partial, size_t partial_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    GDM_CHECK_ARG(scene_rows && model_rows && mask && best_idx && best_sim && col_idx && col_sim && partial,
                  "gdm_match_twoway_packed_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && N >= 1 && M >= 1, "gdm_match_twoway_packed_hip: bad shape B=%d N=%d M=%d", B, N, M);
    GDM_CHECK_ARG((long)B * N < (1L << 22), "gdm_match_twoway_packed_hip: B*N too large");
    GDM_CHECK_ARG(M <= GDM_MATCH_SOFT_MAX_M, "gdm_match_twoway_packed_hip: M=%d, the two-way kernel covers M <= %d", M, GDM_MATCH_SOFT_MAX_M);
    GDM_CHECK_ARG(precision == GDM_MATCH_BF16X3 || precision == GDM_MATCH_F32, "gdm_match_twoway_packed_hip: precision=%d", precision);
    GDM_CHECK_ARG(((uintptr_t)partial & 15) == 0, "gdm_match_twoway_packed_hip: partial must be 16-byte aligned");
    GDM_CHECK_ARG((((uintptr_t)scene_rows | (uintptr_t)model_rows) & 15) == 0, "gdm_match_twoway_packed_hip: the packed rows must be 16-byte aligned");
    const int R = B * N;
    const size_t half = align256(64 * (size_t)R * sizeof(float));
    const size_t nkeys = (size_t)B * M;
    const size_t need = 2 * half + align256(nkeys * sizeof(unsigned long long));
    if (partial_bytes < need) {
        gdm_set_error("gdm_match_twoway_packed_hip: partial workspace %zu < %zu bytes", partial_bytes, need);
        return GDM_ENOMEM;
    }
    float* pval = (float*)partial;
    int32_t* pidx = (int32_t*)((unsigned char*)partial + half);
    unsigned long long* keys = (unsigned long long*)((unsigned char*)partial + 2 * half);
    const int panels = gdm_cdiv(M, PANEL_COLS);
    const int nrb = gdm_cdiv(R, V2_ROWS);
    int G = 512 / panels;                                       // as v2: one workgroup per CU, two rounds
    if (G < 1) G = 1;
    if (G > nrb) G = nrb;
    if (G >= 8) G &= ~7;
    const dim3 kgrid((unsigned)((nkeys + 255) / 256));
    const hipError_t me = hipMemsetAsync(keys, 0, nkeys * sizeof(unsigned long long), stream);      // key 0 = no candidate
    if (me != hipSuccess) {
        gdm_set_error("gdm_match_twoway_packed_hip: hipMemsetAsync of the keys failed: %s", hipGetErrorString(me));
        return (int)me;
    }
    int rc;
    float* ov = panels == 1 ? best_sim : pval;
    int32_t* oi = panels == 1 ? best_idx : pidx;
    gdm_dispatch_int<2>(precision, [&](auto P) {
        constexpr auto kernel = match_panel_twoway_kernel<decltype(P)::value>;
        gdm_allow_lds<kernel>(TWOWAY_LDS_BYTES);
        hipLaunchKernelGGL(kernel, dim3(panels * G), dim3(V2_THREADS), TWOWAY_LDS_BYTES, stream, (const unsigned char*)scene_rows,
                           (const unsigned char*)model_rows, mask, R, N, M, G, ov, oi, keys);
    });
    rc = gdm_launch_status("match_panel_twoway_kernel");
    if (rc) return rc;
    if (panels > 1) {
        hipLaunchKernelGGL(merge_splits_kernel, dim3(gdm_cdiv(R, 256)), dim3(256), 0, stream, pval, pidx, panels, R, best_sim, best_idx);
        rc = gdm_launch_status("merge_splits_kernel");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(twoway_cols_kernel, kgrid, dim3(256), 0, stream, keys, (long)nkeys, col_idx, col_sim);
    return gdm_launch_status("twoway_cols_kernel");
}

extern "C" int gdm_match_cycle_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const int32_t* best_idx,
                                   const int32_t* col_idx, const uint8_t* mask, int B, int N, int M, float radius, uint8_t* pair_mask,
                                   int32_t* pair_count, float* cycle_d2, void* stream)
{
    GDM_CHECK_ARG(scene_xyz && best_idx && col_idx && mask && pair_mask && pair_count && cycle_d2, "gdm_match_cycle_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && N >= 1 && M >= 1, "gdm_match_cycle_hip: bad shape B=%d N=%d M=%d", B, N, M);
    GDM_CHECK_ARG(pt_stride >= 1 && ch_stride >= 1 && scene_bstride >= 0, "gdm_match_cycle_hip: bad scene strides");
    GDM_CHECK_ARG(radius >= 0.f && radius < INFINITY, "gdm_match_cycle_hip: radius=%g must be finite and >= 0", (double)radius);   // a NaN fails
    hipLaunchKernelGGL(match_cycle_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, scene_xyz, scene_bstride, pt_stride, ch_stride,
                       best_idx, col_idx, mask, N, M, radius * radius, pair_mask, pair_count, cycle_d2);
    return gdm_launch_status("match_cycle_kernel");
}

// the dual launch's workspace: the soft launch's (row partials, row sums), then the keys u64[B,M], the column partials
// f32[B * ceil(N / 256), M] and Zc f32[B,M]
extern "C" size_t gdm_match_dual_partial_bytes(int B, int N, int M)
{
    if (B < 1 || N < 1 || M < 1) return 0;
    const size_t cols = (size_t)B * M;
    return gdm_match_soft_partial_bytes(B, N) + align256(cols * sizeof(unsigned long long)) +
           align256(cols * gdm_cdiv(N, V2_ROWS) * sizeof(float)) + align256(cols * sizeof(float));
}

extern "C" int gdm_match_dual_packed_hip(const void* scene_rows, const void* model_rows, const float* model_xyz, const uint8_t* mask, int B,
                                         int N, int M, int precision, float gamma, int32_t* best_idx, float* best_sim, float* lse,
                                         float* conf, float* soft_xyz, int32_t* col_idx, float* col_sim, float* col_lse, float* col_conf,
                                         float* dual, void* partial, size_t partial_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    GDM_CHECK_ARG(scene_rows && model_rows && model_xyz && mask && best_idx && best_sim && lse && conf && soft_xyz && col_idx && col_sim &&
                      col_lse && col_conf && dual && partial,
                  "gdm_match_dual_packed_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && N >= 1 && M >= 1, "gdm_match_dual_packed_hip: bad shape B=%d N=%d M=%d", B, N, M);
    GDM_CHECK_ARG((long)B * N < (1L << 22), "gdm_match_dual_packed_hip: B*N too large");
    GDM_CHECK_ARG(M <= GDM_MATCH_SOFT_MAX_M, "gdm_match_dual_packed_hip: M=%d, the dual kernel covers M <= %d", M, GDM_MATCH_SOFT_MAX_M);
    GDM_CHECK_ARG(precision == GDM_MATCH_BF16X3 || precision == GDM_MATCH_F32, "gdm_match_dual_packed_hip: precision=%d", precision);
    GDM_CHECK_ARG(gamma > 0.f && gamma <= GDM_MATCH_SOFT_MAX_GAMMA, "gdm_match_dual_packed_hip: gamma=%g not in (0, %g]", (double)gamma,
                  (double)GDM_MATCH_SOFT_MAX_GAMMA);                       // a NaN fails both comparisons
    GDM_CHECK_ARG(((uintptr_t)partial & 15) == 0, "gdm_match_dual_packed_hip: partial must be 16-byte aligned");
    GDM_CHECK_ARG((((uintptr_t)scene_rows | (uintptr_t)model_rows) & 15) == 0, "gdm_match_dual_packed_hip: the packed rows must be 16-byte aligned");
    const int R = B * N;
    const int nrbc = gdm_cdiv(N, V2_ROWS);
    const size_t ncols = (size_t)B * M;
    const size_t half = align256(64 * (size_t)R * sizeof(float));
    const size_t sums = align256(64 * (size_t)R * sizeof(float4));
    const size_t kbytes = align256(ncols * sizeof(unsigned long long));
    const size_t cbytes = align256(ncols * nrbc * sizeof(float));
    const size_t need = 2 * half + sums + kbytes + cbytes + align256(ncols * sizeof(float));
    if (partial_bytes < need) {
        gdm_set_error("gdm_match_dual_packed_hip: partial workspace %zu < %zu bytes", partial_bytes, need);
        return GDM_ENOMEM;
    }
    unsigned char* base = (unsigned char*)partial;
    float* pval = (float*)base;
    int32_t* pidx = (int32_t*)(base + half);
    float4* psum = (float4*)(base + 2 * half);
    unsigned long long* keys = (unsigned long long*)(base + 2 * half + sums);
    float* cpart = (float*)(base + 2 * half + sums + kbytes);
    float* zc = (float*)(base + 2 * half + sums + kbytes + cbytes);
    const int panels = gdm_cdiv(M, PANEL_COLS);
    const int nq = B * nrbc;                                    // row blocks: none spans a crop
    int G = 512 / panels;                                       // as v2: one workgroup per CU, two rounds
    if (G < 1) G = 1;
    if (G > nq) G = nq;
    if (G >= 8) G &= ~7;
    const float k2 = gamma * 1.44269504088896340736f;
    const hipError_t me = hipMemsetAsync(keys, 0, ncols * sizeof(unsigned long long), stream);      // key 0 = no candidate
    if (me != hipSuccess) {
        gdm_set_error("gdm_match_dual_packed_hip: hipMemsetAsync of the keys failed: %s", hipGetErrorString(me));
        return (int)me;
    }
    gdm_dispatch_int<2>(precision, [&](auto P) {
        constexpr auto kernel = match_panel_dual_kernel<decltype(P)::value>;
        gdm_allow_lds<kernel>(DUAL_LDS_BYTES);
        hipLaunchKernelGGL(kernel, dim3(panels * G), dim3(V2_THREADS), DUAL_LDS_BYTES, stream, (const unsigned char*)scene_rows,
                           (const unsigned char*)model_rows, model_xyz, mask, B, N, M, G, k2, pval, pidx, psum, keys, cpart);
    });
    int rc = gdm_launch_status("match_panel_dual_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(soft_merge_kernel, dim3(gdm_cdiv(R, 256)), dim3(256), 0, stream, pval, pidx, psum, panels, R, gamma, k2, best_sim,
                       best_idx, lse, conf, soft_xyz);
    rc = gdm_launch_status("soft_merge_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(dual_cols_kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, stream, keys, cpart, (long)ncols, nrbc, M, gamma,
                       k2, col_idx, col_sim, col_lse, col_conf, zc);
    rc = gdm_launch_status("dual_cols_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(dual_rows_kernel, dim3(gdm_cdiv(R, 256)), dim3(256), 0, stream, best_idx, best_sim, conf, mask, zc, R, N, M, k2, dual);
    return gdm_launch_status("dual_rows_kernel");
}

extern "C" int gdm_match_hip(const float* scene, const float* model, int B, int Dd, int N, int M, int precision,
                             int32_t* best_idx, float* best_sim, float* sim,
                             void* workspace, size_t workspace_bytes, void* stream)
{
    GDM_CHECK_ARG(scene && model && best_idx && best_sim && workspace, "gdm_match_hip: NULL pointer");
    GDM_CHECK_ARG(Dd == D, "gdm_match_hip: D=%d, only D=128 is built", Dd);
    GDM_CHECK_ARG(B >= 1 && N >= 1 && M >= 1, "gdm_match_hip: bad shape B=%d N=%d M=%d", B, N, M);
    GDM_CHECK_ARG((long)B * N < (1L << 22), "gdm_match_hip: B*N too large");
    GDM_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "gdm_match_hip: workspace must be 16-byte aligned");
    if (workspace_bytes < gdm_match_workspace_bytes(B, N, M)) {
        gdm_set_error("gdm_match_hip: workspace %zu < %zu bytes", workspace_bytes, gdm_match_workspace_bytes(B, N, M));
        return GDM_ENOMEM;
    }
    unsigned char* ws = (unsigned char*)workspace;
    unsigned char* apk = ws;
    unsigned char* bpk = apk + gdm_match_rows_bytes(B * N);
    unsigned char* part = bpk + gdm_match_rows_bytes(M);
    int rc = gdm_match_pack2_hip(scene, B, N, apk, model, 1, M, bpk, Dd, precision, stream);
    if (rc) return rc;
    return gdm_match_packed_hip(apk, bpk, B * N, M, precision, best_idx, best_sim, sim, part, gdm_match_partial_bytes(B, N), stream);
}
