// 3x3 / stride 1 / pad 1 convolution as an implicit GEMM on split-bf16 MFMA, gfx950.
//
// For the 32x32-resolution half of the ResNet-18 trunk (layer3 / layer4 of
// /root/reference/models/cnn/extractors.py:36-58,151-177: 128..512 -> 256..512 channels), where MIOpen's
// fp32 path is an ASM Winograd F(2,3) kernel on the vector ALUs (~118 TF/s direct-equivalent).  fp32 products are
// replaced by three bf16 MFMAs (hi*hi + hi*lo + lo*hi, fp32 accumulate; |err| <= 3*2^-16 |w x| per product: a bf16 half-ulp is
// 2^-8 relative, so |lo| <= 2^-8 |v|, |v - hi - lo| <= 2^-16 |v|, and the dropped lo*lo and the two residual terms are 2^-16 each;
// the same scheme as the descriptor matching kernel), which is ~5x the f32-MFMA rate.
//
//   out[b,co,y,x] = act( scale[co] * sum_{tap,ci} W[co,ci,tap] * in[b,ci,y+ky-1,x+kx-1] + shift[co] (+ res) )
//
// Data layout: activations are re-packed once per layer (pack kernel below) into bf16 hi / lo planes of 8 channels with a
// one-pixel zero border (fragment-planar: gdm_packed_act.h defines the format), so a tap is just a pixel offset, the zero padding is
// real zeros and every operand load of a wave is two contiguous 512-B runs.  Weights are packed once per weight change into
// rows (tap, chunk, co) of the same 512-B format.  Then the kernel is the matching kernel's shape: a wave keeps
// 32 pixels x 128 channels of one (tap, chunk) in 64 VGPRs as the MFMA A operand, 128 output channels of that
// (tap, chunk) sit in a double-buffered, XOR-swizzled LDS panel as the B operand (global -> registers before the
// MFMAs, registers -> LDS after them, ONE barrier per panel), 9 * Cin/128 panels accumulate into four 32x32 tiles.
#include "gdm_common.h"
#include "gdm_packed_act.h"
#include <math.h>
#include <limits.h>
#include <stdlib.h>

namespace {

constexpr int ROWB = 512;                 // bytes per packed row (128 channels, hi | lo)
static_assert(ROWB == GDM_PK_PLANES * GDM_PK_GRANULE, "a pixel's 128 channels are a row's worth of granules");
constexpr int CV_PIX = 256;               // pixels per workgroup (32 per wave)
constexpr int CV_CO = 128;                // output channels per workgroup
constexpr int CV_PANEL = CV_CO * ROWB;    // 64 KiB
#ifndef GDM_CONV16_PF
#define GDM_CONV16_PF 2
#endif

// x f32[B,C,H,W] -> packed activations (the layout: gdm_packed_act.h)
// one block: 64 consecutive pixels of one image x one 128-channel chunk
__global__ __launch_bounds__(256) void conv_pack_act_kernel(const float* __restrict__ x, int C, int H, int W,
                                                            unsigned char* __restrict__ out)
{
    __shared__ float t[128][65];
    const int b = blockIdx.z, chunk = blockIdx.y;
    const gdm_packed_map pm{C, H, W};
    const int cvalid = min(128, C - chunk * 128);          // a trailing partial chunk: the missing channels' planes stay zero
    const int hw = H * W;
    const int p0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int p = min(p0 + lane, hw - 1);
    const float* xb = x + ((long)b * C + chunk * 128) * hw;
    for (int c = w; c < cvalid; c += 4) t[c][lane] = xb[(long)c * hw + p];
    __syncthreads();
    const int pp = p0 + lane;
    if (pp >= hw) return;
    const int y = pp / W, xx = pp - y * W;
    unsigned char* o = out + pm.pixel(b, chunk, y, xx);
    for (int q = w; q * 8 < cvalid; q += 4) {            // consecutive lanes = consecutive pixels: 1-KiB contiguous stores
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = t[q * 8 + j][lane];
        gdm_packed_store8(o, pm.group(q), pm.group(GDM_PK_LO + q), v);
    }
}

// w f32[Cout,Cin,3,3] -> rows ((tap*nchunk + chunk)*CoutP + co): channels [128 chunk, +128) of tap (ky,kx); CoutP = Cout rounded
// up to 128, rows co >= Cout are zero (a workgroup always stages 128 rows)
// dgrad: w is the FORWARD weight f32[Cin, Cout, taps] of the layer whose input gradient is wanted; the rows written are those of the
// flipped, transposed filter w'[co][ci][tap] = w[ci][co][taps - 1 - tap] (the input gradient of a 3x3/s1/p1 or 1x1 convolution is the same
// convolution of grad_out with w') -- no flip / transpose / contiguous copies in front of the pack.
__global__ __launch_bounds__(256) void conv_pack_w_kernel(const float* __restrict__ w, int Cout, int Cin, int taps, unsigned char* __restrict__ out,
                                                          int dgrad = 0)
{
    const int nchunk = (Cin + 127) / 128;
    const int CoutP = (Cout + 127) & ~127;
    const long item = (long)blockIdx.x * 256 + threadIdx.x;       // (row, 16 groups of 8 channels)
    const long rows = (long)taps * nchunk * CoutP;
    if (item >= rows * 16) return;
    const int ch = (int)(item & 15);
    const long row = item >> 4;
    const int co = (int)(row % CoutP);
    const int tc = (int)(row / CoutP);
    const int chunk = tc % nchunk, tap = tc / nchunk;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = chunk * 128 + ch * 8 + j;
        const bool in = co < Cout && ci < Cin;
        v[j] = !in ? 0.f : dgrad ? w[((long)ci * Cout + co) * taps + (taps - 1 - tap)] : w[((long)co * Cin + ci) * taps + tap];
    }
    gdm_u32x4 hi, lo;
    gdm_split8(v, hi, lo);
    unsigned char* r = out + row * ROWB;
    *reinterpret_cast<gdm_u32x4*>(r + ch * 16) = hi;
    *reinterpret_cast<gdm_u32x4*>(r + 256 + ch * 16) = lo;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same kernel on v_mfma_f32_16x16x32_bf16.  Same workgroup tile (256 pixels x 128 output channels), same panels, same LDS
// image, same operand bytes per MFMA cycle (a wave's 32 x 128 tile is 2 x 8 tiles of 16 x 16; a k-step is 32 channels: two
// A fragments per (hi, lo), eight B fragments); what changes is the lane <-> (row, k-group) map of the fragments and of the
// accumulators.  MI355X holds a visibly higher clock in 16x16x32 loops than in 32x32x16 loops at equal cycles per FLOP
// (MI355X_MICROARCH.md, DVFS item 7: 1.12-1.15x on LDS-fed loops), which is the whole reason for this variant.
//   A fragment (S, ph): lane l -> pixel (l & 15) + 16 ph, channels 8 (4 S + (l >> 4)) .. + 8     = plane 4 S + (l >> 4) of the chunk
//   B fragment (S, cb): lane l -> output channel 16 cb + (l & 15), same channel group            = 16-B chunk 4 S + (l >> 4) of its row
//   accumulator (ph, cb): lane l -> channel 16 cb + (l & 15), pixels 16 ph + 4 (l >> 4) + 0..3   = one 16-byte store
// ---------------------------------------------------------------------------------------------------------------------------
// pixel fragments (16 pixels each) per wave: 2 = eight waves of 32 pixels (two waves per SIMD), 4 = four waves of 64 pixels (one
// wave per SIMD, 512 registers): every B fragment read from LDS then feeds twice the MFMAs and no partner wave competes for the
// matrix pipe; the per-panel barrier joins four waves instead of eight.
#ifndef GDM_CONV_NPH
#define GDM_CONV_NPH 2
#endif
// The MFMAs of a unit are issued accumulator-major.  Product-major issue (no MFMA directly behind the one whose accumulator it reads) was
// measured equal (512 -> 512: 191 vs 188 us on two boxes; the register-only probe gdm_mfma_probe_hip sustained 2.25 PF/s with independent and
// 2.40 PF/s with back-to-back dependent MFMAs at two waves per SIMD): dependent issue was not what idled the pipe.
// k-steps (of the 4 of a 128-channel panel) whose operand reload is deferred to the top of the next panel
#ifndef GDM_CONV16_LATE
#define GDM_CONV16_LATE 1
#endif
constexpr int MF_NPH = GDM_CONV_NPH;
constexpr int MF_WPIX = 16 * MF_NPH;                  // pixels per wave
constexpr int MF_WAVES = CV_PIX / MF_WPIX;
constexpr int MF_THREADS = MF_WAVES * 64;
// Dynamic LDS of a workgroup with NCB 16-channel output blocks: two weight panels, or (packed output) the waves' output tiles of
// NCB * 16 + 4 floats per pixel row (conflict-free reads) where those are larger.  Also the bound every non-GADD instance is allowed.
constexpr int conv_lds_bytes(int NCB)
{
    const int panels = 2 * NCB * 16 * ROWB, tiles = CV_PIX * (NCB * 16 + 4) * 4;
    return panels > tiles ? panels : tiles;
}
constexpr int LDS_MAX = 160 * 1024;                   // a CU's LDS: the bound of the GADD instances, which stage their rows of gt behind the tiles
static_assert(conv_lds_bytes(8) == 135168 && conv_lds_bytes(4) == 69632 && conv_lds_bytes(9) == 151552 && conv_lds_bytes(8) >= 2 * CV_PANEL,
              "at least what every launch site passes");

// NCB = 16-channel output blocks per workgroup: 8 (128 channels) or 4 (64 channels: twice the workgroups for the layers whose 128-channel
// tiling leaves half the chip idle -- layer1-3 of the trunk at batch 16 -- and no zero-padded weight rows for 64-channel layers)
// WV = waves per workgroup: 8 (256 pixels), or 4 (128 pixels: the 128 -> 128 layers at 32 x 32 have 128 workgroups of the 256-pixel, 64-channel
// tiling on 256 CUs -- half tiles put one on every CU)
// GADD (NCHW / packed epilogue only): the point-to-pixel fusion tail in the epilogue -- the GEMM result x takes the gathered point term
// and the folded BatchNorm, out = act(scale[co] * (x + gt[b, co, clamp(gidx[b, pixel])]) + shift[co]), with the bits of the GEMM
// followed by gather_add_affine_act_kernel (gdm_image.hip) and without the fp32 map between them
template <int ACT, bool HAS_RES, int TAPS = 9, bool PIXMAJOR = false, int NKS = 8, int NCB = 8, int WV = MF_WAVES, bool GADD = false>
__global__ __launch_bounds__(MF_THREADS) void conv_mfma16_kernel(const unsigned char* __restrict__ xpk, const unsigned char* __restrict__ wpk,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                                 const float* __restrict__ res, int B, int Cin, int Cout, int H, int W,
                                                                 float* __restrict__ out, const int32_t* __restrict__ rowidx = nullptr,
                                                                 const int32_t* __restrict__ tile_co0 = nullptr,
                                                                 unsigned char* __restrict__ outpk = nullptr, int stride = 1,
                                                                 // per-image weights (the weight-gradient GEMM: image b of a workgroup's 256 pixels --
                                                                 // H*W % 256 == 0 -- reads its rows at wpk + b * wbstride); 0 = shared weights
                                                                 long wbstride = 0,
                                                                 // GADD: gidx int32[B, H*W] (per pixel), gt f32[B, Cout, gn] (channel-major)
                                                                 const int32_t* __restrict__ gidx = nullptr,
                                                                 const float* __restrict__ gt = nullptr, int gn = 0,
                                                                 // byte offset in LDS (behind the panels and the output tile) where the
                                                                 // workgroup stages its rows of gt, gn + 1 floats apart; 0: the lanes
                                                                 // gather from global memory.  Needs one image per workgroup (hw % 256 == 0)
                                                                 int gt_lds = 0)
{
    // H, W: OUTPUT map; the packed input is the (H stride) x (W stride) map (stride 2: layer2's first block, extractors.py:151-177)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // 2 x CV_PANEL
    constexpr int NS = NKS / 2;                                     // k-steps of 32 channels per chunk
    constexpr int UG = (NCB % 2 == 0) ? 2 : 3;                      // 16-channel output blocks per unit (NCB = 9: three)
    constexpr int NPR = NCB / UG;                                   // units per k-step
    constexpr int PANEL = NCB * 16 * ROWB;                          // bytes of a weight panel in LDS
    constexpr int TST = NCB * 16 + 4;                               // floats per pixel row of a wave's output tile in LDS
    static_assert(NCB == 8 || (NCB == 4 && !PIXMAJOR) || (NCB == 9 && !PIXMAJOR && WV == 8),
                  "64-channel tiles: NCHW / packed output only; 144-channel tiles: NCHW fp32 output only (no packed output: a tile straddles 128-channel chunks)");
    constexpr int NPH = MF_NPH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform FOR THE COMPILER too: everything derived from it stays scalar
    const int l16 = lane & 15, kg = lane >> 4;                      // row inside a 16-row fragment, 8-channel group inside a k-step
    const int nchunk = (Cin + 127) / 128;
    const int npanel = TAPS * nchunk;
    const int hw = H * W;
    const long ptot = rowidx ? (long)B : (long)B * hw;              // host: ptot % MF_WPIX == 0 (and hw % MF_WPIX == 0 for maps)
    const unsigned bx = blockIdx.x, by = blockIdx.y;
    const long pix0 = (long)bx * (WV * MF_WPIX) + wave * MF_WPIX;           // this wave's first pixel
    const int co0 = tile_co0 ? __builtin_amdgcn_readfirstlane(tile_co0[bx]) : by * (NCB * 16);
    const long pc = min(pix0, ptot - MF_WPIX);
    const int b = (int)(pc / hw);                                   // one image per wave (hw % MF_WPIX == 0)
    const int prem = (int)(pc - (long)b * hw);
    const int Wi = W * stride;
    // input planes (operand loads): gdm_packed_map{Cin, H stride, Wi}.plane(); the reader keeps its own arithmetic (from the members,
    const long plane = (long)(H * stride + 2) * (Wi + 2);           // the same values compile to other scalar code in every instance)
    const gdm_packed_map om{Cout, H, W};                            // the packed output (packed epilogue)
    // Operand loads are BUFFER loads: descriptor over the packed activations, per-lane byte offset fixed for the whole kernel
    // (plane kg of a k-step + the lane's pixel), everything that changes per panel / tap / k-step in the SCALAR offset.  The flat
    // form recomputed a 64-bit per-lane address for every load (v_mad_u64 / v_lshl_add_u64 / v_mul_lo clumps of ~45 vector
    // instructions at the head of each half panel, issued by both waves of a SIMD at once right behind the barrier: MFMA pipe idle).
    // conv_launch, the only way to this kernel, refuses packed buffers of 2 GiB or more: every offset below is a byte offset INSIDE one
    // of the two buffers, so it fits an int.
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(xpk), (short)0, 0x7ffffff0, 0x00020000);
    int avoff[NPH];                                                 // fragment ph: 16 consecutive pixels of one image row (W % 16 == 0)
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph) {
        const int pr = prem + 16 * ph;
        const int yy = pr / W, xx = pr - yy * W;
        const long pixbase = rowidx ? (long)max(rowidx[pc + l16 + 16 * ph], 0) : (long)(yy * stride) * (Wi + 2) + (long)(xx + l16) * stride;
        avoff[ph] = (int)(((long)kg * plane + pixbase) * GDM_PK_GRANULE);
    }

    gdm_u32x4 ahi[NS][NPH], alo[NS][NPH];                               // fragments of k-step S, pixel fragment ph
    // Panel bookkeeping in scalar registers, advanced by counters (no division in the loop): panel = (chunk, ky, kx), chunk-major
    // (the nine taps of a chunk back to back).  pan_a / pan_w: byte offsets of a panel's operand rows / weight rows.
    struct Pan { int chunk, ky, kx; };
    auto pan_next = [&](Pan p) -> Pan {
        if (TAPS == 1) { ++p.chunk; return p; }
        if (++p.kx == 3) { p.kx = 0; if (++p.ky == 3) { p.ky = 0; ++p.chunk; } }
        return p;
    };
    const int a_base = (int)(((long)(rowidx ? 0 : b) * nchunk * GDM_PK_PLANES) * plane * GDM_PK_GRANULE);
    const int a_chunk = (int)(GDM_PK_PLANES * plane * GDM_PK_GRANULE), a_rowb = (Wi + 2) * GDM_PK_GRANULE;
    auto pan_a = [&](Pan p) -> int { return a_base + p.chunk * a_chunk + p.ky * a_rowb + p.kx * GDM_PK_GRANULE; };
    const int sstride = (int)(4 * plane * GDM_PK_GRANULE);          // plane 4 S + kg -> 4 (S + 1) + kg
    const int lostride = (int)(GDM_PK_LO * plane * GDM_PK_GRANULE); // hi plane q -> lo plane 16 + q
    auto load_a = [&](int r, int S) {
#pragma unroll
        for (int ph = 0; ph < NPH; ++ph) {
            ahi[S][ph] = __builtin_bit_cast(gdm_u32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, avoff[ph], r + S * sstride, 0));
            alo[S][ph] = __builtin_bit_cast(gdm_u32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, avoff[ph], r + S * sstride + lostride, 0));
        }
    };
    // a weight panel is staged in two halves (global -> registers -> LDS), each half in flight for half a panel: 16 registers
    constexpr int THREADS = WV * 64, WGPIX = WV * MF_WPIX;
    constexpr int HS = (NCB * 512 / THREADS) / 2;
    gdm_u32x4 stage[HS];
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(wpk), (short)0, 0x7ffffff0, 0x00020000);
    const int w_base = (wbstride ? (int)(((long)bx * WGPIX / hw) * wbstride) : 0) + co0 * ROWB;
    const int w_panel = ((Cout + 127) & ~127) * ROWB;               // the packed weights are (tap, chunk, co) rows
    auto pan_w = [&](Pan p) -> int { return w_base + ((TAPS == 1) ? p.chunk : (p.ky * 3 + p.kx) * nchunk + p.chunk) * w_panel; };
    auto stage_load = [&](int src, int half) {
#pragma unroll
        for (int i = 0; i < HS; ++i)
            stage[i] = __builtin_bit_cast(gdm_u32x4, __builtin_amdgcn_raw_buffer_load_b128(wr, tid * 16, src + (half * HS + i) * THREADS * 16, 0));
    };
    auto stage_store = [&](int buf, int half) {
        unsigned char* base = smem + buf * PANEL;
#pragma unroll
        for (int i = 0; i < HS; ++i) {
            const int g = (half * HS + i) * THREADS + tid;
            *reinterpret_cast<gdm_u32x4*>(base + gdm_swz<ROWB>(g >> 5, g & 31)) = stage[i];
        }
    };
    // GLDS (eight-wave workgroups; the four-wave half tiles stage through registers, above): the weight panel goes global -> LDS by LDS-DMA (buffer_load ... lds), no staging registers and no
    // ds_write pass.  A wave instruction fills 1 KiB = two 512-byte rows LINEARLY (LDS address = M0 base + lane * 16), so the XOR
    // swizzle of the LDS image sits on the per-lane SOURCE offset: lane p of piece j = 8 i + wave writes slot p & 31 of row
    // col = 2 j + (p >> 5), which must hold chunk ch = (s & 16) | ((s ^ col) & 15) of that row (gdm_swz is an involution); 2 j = 16 i + 2 wave,
    // so col & 15 -- and with it the lane's source offset -- is the same for every piece of a wave.
    constexpr bool GLDS = WV == 8;
    constexpr int NPIECE = PANEL / 1024 / 8;                        // LDS-DMA instructions per wave and panel
    int glds_voff = 0;
    if (GLDS) {
        const int hrow = lane >> 5, sl = lane & 31;
        const int col15 = (2 * wave + hrow) & 15;
        glds_voff = wave * 1024 + hrow * 512 + (((sl & 16) | ((sl ^ col15) & 15)) << 4);
    }
    typedef __attribute__((address_space(3))) void* lds_void_ptr;
    auto stage_glds = [&](int src, int buf) {
#pragma unroll
        for (int i = 0; i < NPIECE; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void_ptr)(smem + buf * PANEL + (i * 8 + wave) * 1024), 16, glds_voff, src + i * 8192, 0, 0);
    };

    gdm_f32x4 acc[NPH][NCB];
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[ph][cb][i] = 0.f;

    constexpr int LATE = GDM_CONV16_LATE < NS ? GDM_CONV16_LATE : NS;                           // k-steps whose reload is deferred to the next iteration's top
    Pan pcur = {0, (TAPS == 1) ? 1 : 0, (TAPS == 1) ? 1 : 0};
    if (GLDS) {
        stage_glds(pan_w(pcur), 0);
    } else {
        stage_load(pan_w(pcur), 0);
        stage_store(0, 0);
        stage_load(pan_w(pcur), 1);
        stage_store(0, 1);
    }
    int rcur = pan_a(pcur);
#pragma unroll
    for (int S = 0; S < NS - LATE; ++S) load_a(rcur, S);
    Pan pnxt = npanel > 1 ? pan_next(pcur) : pcur;
    int rnext = pan_a(pnxt), wnext = pan_w(pnxt);                   // (a harmless re-read of the same rows behind the last panel)
    for (int it = 0; it < npanel; ++it) {
        __syncthreads();                                            // panel `it` is in LDS; panel it-1's readers are done
        const bool more = it + 1 < npanel;
        const unsigned char* base = smem + (it & 1) * PANEL;
        // units of (k-step S, UG 16-channel output blocks): 3 UG NPH MFMAs of 16 cycles on 2 UG B fragments; PF units' reads in flight
        constexpr int PF = GDM_CONV16_PF;
        constexpr int NU = NPR * NS;
        gdm_u32x4 fh[PF + 1][UG], fl[PF + 1][UG];
        auto frag_load = [&](int un) {
            const int S = un / NPR, pr = un % NPR, slot = un % (PF + 1);
#pragma unroll
            for (int j = 0; j < UG; ++j) {
                const int col = (UG * pr + j) * 16 + l16;
                fh[slot][j] = *reinterpret_cast<const gdm_u32x4*>(base + gdm_swz<ROWB>(col, 4 * S + kg));
                fl[slot][j] = *reinterpret_cast<const gdm_u32x4*>(base + gdm_swz<ROWB>(col, 16 + 4 * S + kg));
            }
        };
#pragma unroll
        for (int un = 0; un < PF; ++un) frag_load(un);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int S = u / NPR, pr = u % NPR, slot = u % (PF + 1);
            if (u + PF < NU) frag_load(u + PF);
#pragma unroll
            for (int ph = 0; ph < NPH; ++ph) {
                const gdm_bf16x8 ah = __builtin_bit_cast(gdm_bf16x8, ahi[S][ph]);
                const gdm_bf16x8 al = __builtin_bit_cast(gdm_bf16x8, alo[S][ph]);
#pragma unroll
                for (int j = 0; j < UG; ++j) {
                    gdm_f32x4 c = acc[ph][UG * pr + j];
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, __builtin_bit_cast(gdm_bf16x8, fl[slot][j]), c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, __builtin_bit_cast(gdm_bf16x8, fh[slot][j]), c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, __builtin_bit_cast(gdm_bf16x8, fh[slot][j]), c, 0, 0, 0);
                    acc[ph][UG * pr + j] = c;
                }
            }
            if (pr == NPR - 1 && S < NS - LATE) load_a(rnext, S);         // this k-step's registers are dead: next panel's data
            if (!GLDS && u == NU / 2 && more) {                     // the other buffer's readers finished at this panel's barrier
                stage_store((it + 1) & 1, 0);
                stage_load(wnext, 1);
            }
            if (u == 0) {
                if (more) { if (GLDS) stage_glds(wnext, (it + 1) & 1); else stage_load(wnext, 0); }
#pragma unroll
                for (int S2 = NS - LATE; S2 < NS; ++S2) load_a(rcur, S2);
            }
#pragma unroll
            for (int i = 0; i < 3 * UG * NPH; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (u + PF < NU && (i % NPH) == 0 && i < 2 * UG * NPH) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!GLDS && more) stage_store((it + 1) & 1, 1);
        // the next panels' scalar offsets, formed here -- behind the panel's last MFMA, in front of the barrier -- instead of at the
        // head of the next panel, where both waves of a SIMD would run the same ~40 scalar instructions with the matrix pipe idle
        rcur = rnext;
        if (it + 2 < npanel) pnxt = pan_next(pnxt);
        rnext = pan_a(pnxt);
        wnext = pan_w(pnxt);
    }

    // ---- epilogue: lane = output channel 16 cb + l16, registers = 4 consecutive pixels 16 ph + 4 kg + r ----
    if (pix0 >= ptot) return;
    if (PIXMAJOR) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const int co = co0 + cb * 16 + l16;
            if (co >= Cout) continue;
            const float sc = scale ? scale[co] : 1.f, sh = shift ? shift[co] : 0.f;
            const int ocol = tile_co0 ? cb * 16 + l16 : co;
            const int ostride = tile_co0 ? CV_CO : Cout;
#pragma unroll
            for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[ph][cb][r] * sc + sh;
                    if (ACT == 1) v = fmaxf(v, 0.f);
                    out[(pix0 + 16 * ph + 4 * kg + r) * ostride + ocol] = v;
                }
        }
        return;
    }
    // GADD: what the epilogue reads from memory -- the four pixels' indices per ph, the folded BN pair per 16-channel block, the gathered
    // values -- is requested here, in front of the barrier, without a branch in between (rows beyond Cout read row Cout - 1 and are masked
    // below).  The gathered values are NCB * 4 NPH scattered 4-byte loads per lane; a scattered load costs the vector memory pipe a
    // cycle per lane whatever the cache holds (measured: 12 us per workgroup on top of the GEMM, the same with every index 0), so with
    // gt_lds the workgroup copies its NCB * 16 rows of gt (contiguous in memory: coalesced loads) to LDS and gathers there.
    float gtv[GADD ? NPH : 1][GADD ? NCB : 1][4], gsc[GADD ? NCB : 1], gsh[GADD ? NCB : 1];
    int gsrc[GADD ? NPH : 1][4];
    if constexpr (GADD) {
#pragma unroll
        for (int ph = 0; ph < NPH; ++ph) {                           // one 16-byte load (hw % 32 == 0, prem % 32 == 0: aligned)
            const int4 i4 = *reinterpret_cast<const int4*>(gidx + (long)b * hw + prem + 16 * ph + 4 * kg);
            gsrc[ph][0] = min(max(i4.x, 0), gn - 1);
            gsrc[ph][1] = min(max(i4.y, 0), gn - 1);
            gsrc[ph][2] = min(max(i4.z, 0), gn - 1);
            gsrc[ph][3] = min(max(i4.w, 0), gn - 1);
        }
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const int cl = min(co0 + cb * 16 + l16, Cout - 1);
            gsc[cb] = scale[cl];
            gsh[cb] = shift[cl];
        }
        if (gt_lds) {
            float* ts = reinterpret_cast<float*>(smem + gt_lds);
            for (int r = wave; r < NCB * 16; r += WV) {              // a row per wave and turn: gn consecutive floats
                const float* tp = gt + ((long)b * Cout + min(co0 + r, Cout - 1)) * gn;
                for (int c = lane; c < gn; c += 64) ts[r * (gn + 1) + c] = tp[c];
            }
        } else {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const float* tp = gt + ((long)b * Cout + min(co0 + cb * 16 + l16, Cout - 1)) * gn;
#pragma unroll
                for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
                    for (int j = 0; j < 4; ++j) gtv[ph][cb][j] = tp[gsrc[ph][j]];
            }
        }
    }
    float* tl = reinterpret_cast<float*>(smem) + wave * MF_WPIX * TST;
    if (outpk || (GADD && gt_lds)) __syncthreads();                  // every wave has finished reading the last weight panel
    if constexpr (GADD) {
        if (gt_lds) {                                                // (the barrier above: the staged rows are complete)
            const float* ts = reinterpret_cast<const float*>(smem + gt_lds);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
                    for (int j = 0; j < 4; ++j) gtv[ph][cb][j] = ts[(cb * 16 + l16) * (gn + 1) + gsrc[ph][j]];
        }
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        const int co = co0 + cb * 16 + l16;
        const bool live = co < Cout;
        float sc, sh;
        if constexpr (GADD) { sc = gsc[cb]; sh = gsh[cb]; }
        else { sc = (live && scale) ? scale[co] : 1.f; sh = (live && shift) ? shift[co] : 0.f; }
        float* op = out ? out + ((long)b * Cout + (live ? co : 0)) * hw + prem : nullptr;
        const float* rp = (HAS_RES && live) ? res + ((long)b * Cout + co) * hw + prem : nullptr;
#pragma unroll
        for (int ph = 0; ph < NPH; ++ph) {
            const int poff = 16 * ph + 4 * kg;
            float v[4];
            if constexpr (GADD) {
                // the two-launch form's arithmetic, step by step (-ffp-contract=off: the source order is the bit pattern): the GEMM's
                // identity scale / shift (x * 1 + 0: -0 becomes +0), then scale * (x + t) + shift
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x = acc[ph][cb][j] * 1.f + 0.f;
                    v[j] = (x + gtv[ph][cb][j]) * sc + sh;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[ph][cb][j] * sc + sh;
            }
            if (HAS_RES && live) {
                const float4 r4 = *reinterpret_cast<const float4*>(rp + poff);
                v[0] += r4.x; v[1] += r4.y; v[2] += r4.z; v[3] += r4.w;
            }
            if (ACT == 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
            }
            if (op && live) *reinterpret_cast<float4*>(op + poff) = make_float4(v[0], v[1], v[2], v[3]);
            if (outpk) {
#pragma unroll
                for (int j = 0; j < 4; ++j) tl[(poff + j) * TST + cb * 16 + l16] = live ? v[j] : 0.f;
            }
        }
    }
    if (outpk) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int lr = lane & 31, h = lane >> 5;
        const int ochunk = co0 / 128;
#pragma unroll
        for (int half = 0; half < MF_WPIX / 32; ++half) {
            const int pp = prem + 32 * half + lr;                    // this lane's pixel of the wave's tile
            const int yy = pp / W, xx = pp - yy * W;
            unsigned char* ob = outpk + om.pixel(b, ochunk, yy, xx);
            const float* row = tl + (32 * half + lr) * TST;
#pragma unroll
            for (int it = 0; it < NCB; ++it) {
                const int ql = 2 * it + h;                           // 8-channel group inside this workgroup's channels
                if (co0 + ql * 8 >= Cout) continue;
                const int q = (co0 % 128) / 8 + ql;                  // ... and inside the 128-channel chunk of the packed output
                const float4 a0 = *reinterpret_cast<const float4*>(row + ql * 8);
                const float4 a1 = *reinterpret_cast<const float4*>(row + ql * 8 + 4);
                const float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                gdm_packed_store8(ob, om.group(q), om.group(GDM_PK_LO + q), v);
            }
        }
    }
}

// What conv_mfma16_kernel takes, by name and in its order (host side only: conv_launch expands it into the kernel's positional parameters).
struct ConvArgs {
    const void *xpk = nullptr, *wpk = nullptr;
    const float *scale = nullptr, *shift = nullptr, *res = nullptr;
    int B = 0, Cin = 0, Cout = 0, H = 0, W = 0;
    float* out = nullptr;
    const int32_t *rowidx = nullptr, *tile_co0 = nullptr;
    void* outpk = nullptr;
    int stride = 1;
    long wbstride = 0;
    const int32_t* gidx = nullptr;
    const float* gt = nullptr;
    int gn = 0, gt_lds = 0;
    const char* who = "conv_mfma16_kernel";         // the entry point, for the messages of conv_launch
};

// a * b for byte counts, saturating: a refusal must not depend on a product that wrapped
static long mul_sat(long a, long b)
{
    long r;
    return (a < 0 || b < 0 || __builtin_mul_overflow(a, b, &r)) ? LONG_MAX : r;
}

// The one place conv_mfma16_kernel is launched from.  smem is what the SITE wants (it decides how many workgroups share a CU); what the
// instance is allowed is set here, once, so an instance cannot be launched without it.
// The kernel addresses both packed operands through buffer descriptors with 32-bit byte offsets, so each must stay below 2 GiB: checked
// here too, before the first HIP call, from what the kernel itself derives its offsets from -- the activations are the zero-bordered
// (H stride) x (W stride) input map of B images (the grouped form: ONE 1 x W map, B counts gathered rows), the weights TAPS panels per
// 128-channel chunk, behind (B - 1) * wbstride bytes where every image has its own.  Nonzero: refused, gdm_last_error() says why.
// (The alignment of the two pointers is checked behind the limit, so a caller -- a test without a GPU, say -- can see that a shape passed
// the limit without launching it.)
template <int ACT, bool RES, int TAPS, bool PM, int NKS, int NCB, int WV, bool GADD>
int conv_launch(dim3 grid, int smem, hipStream_t s, const ConvArgs& a)
{
    const long chunks = (a.Cin + 127) / 128;
    const long xbytes = mul_sat(mul_sat(a.rowidx ? 1 : a.B, mul_sat((long)a.H * a.stride + 2, (long)a.W * a.stride + 2)), chunks * ROWB);
    const long wpanels = mul_sat(TAPS * chunks, (((long)a.Cout + 127) & ~127L) * ROWB);
    const long wlead = a.wbstride ? mul_sat(a.B - 1, a.wbstride) : 0;
    const long wbytes = wlead > LONG_MAX - wpanels ? LONG_MAX : wlead + wpanels;
    GDM_CHECK_ARG(xbytes < (1L << 31) && wbytes < (1L << 31),
                  "%s: packed operands must stay below 2 GiB (activations %ld bytes, weights %ld bytes)", a.who, xbytes, wbytes);
    // every operand load is 16 bytes wide, and so is every store of the pack kernels that write these buffers
    GDM_CHECK_ARG((((uintptr_t)a.xpk | (uintptr_t)a.wpk) & 15) == 0,
                  "%s: the packed operands must be 16-byte aligned (xpk %p, wpk %p)", a.who, a.xpk, a.wpk);
    // the epilogue adds the residual and stores the result four pixels (or four channels) at a time
    GDM_CHECK_ARG((((uintptr_t)a.res | (uintptr_t)a.out) & 15) == 0, "%s: res and out must be 16-byte aligned (res %p, out %p)", a.who,
                  (const void*)a.res, (const void*)a.out);
    constexpr auto kernel = conv_mfma16_kernel<ACT, RES, TAPS, PM, NKS, NCB, WV, GADD>;
    gdm_allow_lds<kernel>(GADD ? LDS_MAX : conv_lds_bytes(NCB));
    hipLaunchKernelGGL(kernel, grid, dim3(WV * 64), smem, s, (const unsigned char*)a.xpk, (const unsigned char*)a.wpk, a.scale, a.shift, a.res,
                       a.B, a.Cin, a.Cout, a.H, a.W, a.out, a.rowidx, a.tile_co0, (unsigned char*)a.outpk, a.stride, a.wbstride, a.gidx, a.gt,
                       a.gn, a.gt_lds);
    return 0;
}

} // namespace

// Measurement aid (bench.py): what the matrix pipe sustains on THIS chip with nothing else in the way -- every wave issues `iters` x 8
// independent v_mfma_f32_16x16x32_bf16 on registers (no LDS, no memory), eight waves per CU like the convolution kernel.  The chip lowers
// its clock under such a load (MI355X_MICROARCH.md, DVFS), so this -- not the 2.5 PFLOP/s of the data sheet clock -- is the ceiling an
// MFMA-bound kernel can be compared with on the box it runs on.
namespace {
template <int CHAIN>
__global__ __launch_bounds__(512) void mfma_probe_kernel(int iters, float* __restrict__ sink)
{
    const int lane = threadIdx.x & 63;
    gdm_f32x4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = gdm_f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned seed = 0x3f803f80u + (unsigned)lane;             // bf16 pairs near 1.0
    gdm_u32x4 av = {seed, seed ^ 1u, seed ^ 2u, seed ^ 3u}, bv = {seed ^ 4u, seed ^ 5u, seed ^ 6u, seed ^ 7u};
    const gdm_bf16x8 a = __builtin_bit_cast(gdm_bf16x8, av), b = __builtin_bit_cast(gdm_bf16x8, bv);
    // CHAIN consecutive MFMAs into the same accumulator before moving to the next one (1: every MFMA independent of its predecessor;
    // 3: the hi.lo / lo.hi / hi.hi triple of a split-bf16 product issued back to back)
    for (int it = 0; it < iters; it += CHAIN) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < CHAIN; ++c) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i], 0, 0, 0);
    }
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (t == 12345.678f) sink[0] = t;                               // keeps the loop alive; never true
}
// The same with the B operands re-read from LDS at the convolution kernel's ratio: per unit of 12 MFMAs (four accumulators x the three
// split products) four ds_read_b128 of 64 consecutive 16-byte chunks (conflict-free); RPU = reads per unit (4 = the kernel's, 2, 1).
template <int RPU>
__global__ __launch_bounds__(512) void mfma_probe_lds_kernel(int iters, float* __restrict__ sink)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pl[];          // 64 KiB
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < 4096; i += 512) reinterpret_cast<gdm_u32x4*>(pl)[i] = gdm_u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u + (unsigned)i};
    __syncthreads();
    gdm_f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = gdm_f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned seed = 0x3f803f80u + (unsigned)lane;
    gdm_u32x4 a0 = {seed, seed ^ 1u, seed ^ 2u, seed ^ 3u}, a1 = {seed ^ 4u, seed ^ 5u, seed ^ 6u, seed ^ 7u};
    gdm_u32x4 f[4] = {a0, a1, a0, a1};
    int off = lane * 16;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < RPU; ++r) f[r] = *reinterpret_cast<const gdm_u32x4*>(pl + ((off + r * 1024) & 0xffff));
        off += 4096;
#pragma unroll
        for (int prod = 0; prod < 3; ++prod)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gdm_bf16x8, prod == 1 ? a1 : a0),
                                                                 __builtin_bit_cast(gdm_bf16x8, f[(i + prod) & 3]), acc[i], 0, 0, 0);
    }
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) t += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (t == 12345.678f) sink[0] = t;
}
} // namespace

// LDS-fed probe: flops of one launch = blocks * 8 waves * iters * 12 MFMAs * 16384; rpu = ds_read_b128 per 12 MFMAs (1, 2 or 4)
extern "C" int gdm_mfma_probe_lds_hip(int blocks, int iters, int rpu, float* sink, void* stream)
{
    GDM_CHECK_ARG(blocks >= 1 && blocks <= 65535 && iters >= 1 && (rpu == 1 || rpu == 2 || rpu == 4) && sink, "gdm_mfma_probe_lds_hip: bad arguments");
    if (rpu == 4) hipLaunchKernelGGL(mfma_probe_lds_kernel<4>, dim3(blocks), dim3(512), 65536, (hipStream_t)stream, iters, sink);
    else if (rpu == 2) hipLaunchKernelGGL(mfma_probe_lds_kernel<2>, dim3(blocks), dim3(512), 65536, (hipStream_t)stream, iters, sink);
    else hipLaunchKernelGGL(mfma_probe_lds_kernel<1>, dim3(blocks), dim3(512), 65536, (hipStream_t)stream, iters, sink);
    return gdm_launch_status("mfma_probe_lds_kernel");
}

// flops of one launch = blocks * 8 waves * iters * 8 MFMAs * 16*16*32*2
extern "C" int gdm_mfma_probe_hip(int blocks, int iters, int chain, float* sink, void* stream)
{
    GDM_CHECK_ARG(blocks >= 1 && blocks <= 65535 && iters >= 3 && iters % 3 == 0 && (chain == 1 || chain == 3) && sink,
                  "gdm_mfma_probe_hip: bad arguments (iters a multiple of 3, chain 1 or 3)");
    if (chain == 3) hipLaunchKernelGGL(mfma_probe_kernel<3>, dim3(blocks), dim3(512), 0, (hipStream_t)stream, iters, sink);
    else hipLaunchKernelGGL(mfma_probe_kernel<1>, dim3(blocks), dim3(512), 0, (hipStream_t)stream, iters, sink);
    return gdm_launch_status("mfma_probe_kernel");
}

static bool cin_ok(int Cin) { return gdm_packed_channels_ok(Cin); }

// 64-channel output tiles instead of 128-channel ones: when the 128-channel tiling gives fewer workgroups than the chip has CUs, or
// the layer has only 64 output channels
static bool narrow_tiles(unsigned pixel_tiles, int Cout)
{
    return Cout <= 64 || (long)pixel_tiles * ((Cout + 127) / 128) < 256;
}

extern "C" size_t gdm_conv3x3_act_bytes(int B, int Cin, int H, int W)
{
    if (B < 1 || !cin_ok(Cin) || H < 1 || W < 1) return 0;
    return gdm_packed_map{Cin, H, W}.bytes(B);
}

extern "C" size_t gdm_conv3x3_weight_bytes(int Cout, int Cin)
{
    if (Cout < 1 || !cin_ok(Cin)) return 0;
    return (size_t)9 * ((Cin + 127) / 128) * ((Cout + 127) & ~127) * ROWB;
}

extern "C" size_t gdm_conv1x1_weight_bytes(int Cout, int Cin)
{
    if (Cout < 1 || !cin_ok(Cin)) return 0;
    return (size_t)((Cin + 127) / 128) * ((Cout + 127) & ~127) * ROWB;
}

static int pack_weight(const float* w, int Cout, int Cin, int taps, void* wpk, void* stream, const char* who, int dgrad = 0)
{
    GDM_CHECK_ARG(w && wpk, "%s: NULL pointer", who);
    GDM_CHECK_ARG(Cout >= 1 && cin_ok(Cin), "%s: Cout=%d Cin=%d (Cin a multiple of 128, or 64)", who, Cout, Cin);
    const long items = (long)taps * ((Cin + 127) / 128) * ((Cout + 127) & ~127) * 16;
    hipLaunchKernelGGL(conv_pack_w_kernel, dim3(gdm_cdiv(items, 256)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin, taps, (unsigned char*)wpk, dgrad);
    return gdm_launch_status("conv_pack_w_kernel");
}

// The packed weights of the INPUT-GRADIENT convolution straight from the forward weight w f32[Cout, Cin, taps] (taps 9 or 1): the packed
// layer has Cin output channels and Cout input channels (Cout a multiple of 128, or 64); wpk: gdm_conv3x3_weight_bytes(Cin, Cout) /
// gdm_conv1x1_weight_bytes(Cin, Cout) bytes.
extern "C" int gdm_conv_pack_weight_dgrad_hip(const float* w, int Cout, int Cin, int taps, void* wpk, void* stream)
{
    GDM_CHECK_ARG(taps == 9 || taps == 1, "gdm_conv_pack_weight_dgrad_hip: taps=%d (9 or 1)", taps);
    return pack_weight(w, Cin, Cout, taps, wpk, stream, "gdm_conv_pack_weight_dgrad_hip", 1);
}

extern "C" int gdm_conv3x3_pack_weight_hip(const float* w, int Cout, int Cin, void* wpk, void* stream)
{
    return pack_weight(w, Cout, Cin, 9, wpk, stream, "gdm_conv3x3_pack_weight_hip");
}

extern "C" int gdm_conv1x1_pack_weight_hip(const float* w, int Cout, int Cin, void* wpk, void* stream)
{
    return pack_weight(w, Cout, Cin, 1, wpk, stream, "gdm_conv1x1_pack_weight_hip");
}

// xpk must be zero-filled by the caller (the border rows are never written).
extern "C" int gdm_conv3x3_pack_act_hip(const float* x, int B, int Cin, int H, int W, void* xpk, void* stream)
{
    GDM_CHECK_ARG(x && xpk, "gdm_conv3x3_pack_act_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && B <= 65535 && cin_ok(Cin) && H >= 1 && W >= 1, "gdm_conv3x3_pack_act_hip: bad shape (Cin=%d: a multiple of 128, or 64)", Cin);
    dim3 grid(gdm_cdiv((long)H * W, 64), (Cin + 127) / 128, B);
    hipLaunchKernelGGL(conv_pack_act_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, Cin, H, W, (unsigned char*)xpk);
    return gdm_launch_status("conv_pack_act_kernel");
}

// out (fp32 NCHW) and / or outpk (the packed operand of the next convolution over [B, Cout, H, W]; zero-filled once by the caller, only
// interior pixels are written) -- at least one of them.
static int conv3x3_launch(const void* xpk, const void* wpk, const float* scale, const float* shift, const float* res,
                          int B, int Cin, int Cout, int H, int W, int stride, int act, float* out, void* outpk, void* stream,
                          const char* who)
{
    GDM_CHECK_ARG(stride == 1 || stride == 2, "%s: stride=%d (1 or 2)", who, stride);
    GDM_CHECK_ARG(xpk && wpk && (out || outpk), "%s: NULL pointer", who);
    GDM_CHECK_ARG(B >= 1 && cin_ok(Cin) && Cout >= 1, "%s: Cin=%d Cout=%d (Cin a multiple of 128, or 64)", who, Cin, Cout);
    GDM_CHECK_ARG(W % 32 == 0 && H >= 1 && (H * W) % MF_WPIX == 0,
                  "%s: W=%d must be a multiple of 32 and H*W=%d of %d", who, W, H * W, MF_WPIX);
    GDM_CHECK_ARG(act == 0 || act == 1, "%s: act=%d", who, act);
    GDM_CHECK_ARG(!outpk || (Cout % 8 == 0 && ((long)B * H * W) % CV_PIX == 0),
                  "%s: packed output needs Cout %% 8 == 0 and B*H*W %% 256 == 0 (got Cout=%d, B*H*W=%ld)", who, Cout, (long)B * H * W);
    const long ptot = (long)B * H * W;
    const dim3 grid(gdm_cdiv(ptot, CV_PIX), gdm_cdiv(Cout, CV_CO));
    // 64-channel tiles where 128-channel ones leave the chip half empty (or pad a 64-channel layer with zero rows): twice the workgroups
    const bool narrow = narrow_tiles(grid.x, Cout);
    const dim3 grid4(grid.x, gdm_cdiv(Cout, 64));
    // still fewer workgroups than CUs (128 -> 128 at 32 x 32, batch 16: 64 x 2): 128-pixel workgroups of four waves
    const bool half = narrow && Cin != 64 && (long)grid4.x * grid4.y < 256 && ptot % (CV_PIX / 2) == 0;
    const dim3 grid4h(gdm_cdiv(ptot, CV_PIX / 2), grid4.y);
    hipStream_t s = (hipStream_t)stream;
    ConvArgs a{xpk, wpk, scale, shift, res, B, Cin, Cout, H, W, out};
    a.outpk = outpk; a.stride = stride; a.who = who;
    int refused = 0;
    gdm_dispatch_int<2>(act, [&](auto A) {
        gdm_dispatch_bool(res != nullptr, [&](auto R) {
            constexpr int ACT = decltype(A)::value;
            constexpr bool RES = decltype(R)::value;
            if (half) { refused = conv_launch<ACT, RES, 9, false, 8, 4, MF_WAVES / 2, false>(grid4h, conv_lds_bytes(4), s, a); return; }
            gdm_dispatch_bool(Cin == 64, [&](auto K4) {         // one half-filled chunk: only its four non-zero k-steps are run
                constexpr int NKS = decltype(K4)::value ? 4 : 8;
                if (narrow) refused = conv_launch<ACT, RES, 9, false, NKS, 4, MF_WAVES, false>(grid4, conv_lds_bytes(4), s, a);
                else refused = conv_launch<ACT, RES, 9, false, NKS, 8, MF_WAVES, false>(grid, conv_lds_bytes(8), s, a);
            });
        });
    });
    if (refused) return refused;
    return gdm_launch_status(half ? "conv_mfma16_kernel (3x3, 64-channel tiles, 128 pixels)"
                             : narrow ? "conv_mfma16_kernel (3x3, 64-channel tiles)" : "conv_mfma16_kernel (3x3)");
}

extern "C" int gdm_conv3x3_packed_hip(const void* xpk, const void* wpk, const float* scale, const float* shift, const float* res,
                                      int B, int Cin, int Cout, int H, int W, int act, float* out, void* stream)
{
    return conv3x3_launch(xpk, wpk, scale, shift, res, B, Cin, Cout, H, W, 1, act, out, nullptr, stream, "gdm_conv3x3_packed_hip");
}

// H, W = OUTPUT size; xpk = the (H stride) x (W stride) input packed by gdm_conv3x3_pack_act_hip; stride 1 or 2
extern "C" int gdm_conv3x3_strided_hip(const void* xpk, const void* wpk, const float* scale, const float* shift, const float* res,
                                       int B, int Cin, int Cout, int H, int W, int stride, int act, float* out, void* outpk, void* stream)
{
    return conv3x3_launch(xpk, wpk, scale, shift, res, B, Cin, Cout, H, W, stride, act, out, outpk, stream, "gdm_conv3x3_strided_hip");
}

// Grouped, gathered GEMM on the same kernel: Y[r, 0:128] = Wpk[tile_co0[r / 256] + 0:128, :] . X[rowidx[r], :] for R rows (R % 256 == 0),
// X packed by gdm_conv3x3_pack_act_hip(x, 1, Cin, 1, M), weights packed by gdm_conv1x1_pack_weight_hip(Cout_total, Cin).
extern "C" int gdm_gemm_grouped_hip(const void* xpk, const void* wpk, const int32_t* rowidx, const int32_t* tile_co0, int R, int M,
                                    int Cin, int Cout_total, float* out, void* stream)
{
    GDM_CHECK_ARG(xpk && wpk && rowidx && tile_co0 && out, "gdm_gemm_grouped_hip: NULL pointer");
    GDM_CHECK_ARG(R >= 256 && R % 256 == 0 && M >= 1 && Cin >= 128 && Cin % 128 == 0 && Cout_total >= 128 && Cout_total % 128 == 0,
                  "gdm_gemm_grouped_hip: R=%d (multiple of 256) M=%d Cin=%d Cout_total=%d (multiples of 128)", R, M, Cin, Cout_total);
    // the kernel sees B = R "pixels" of a 1 x 1 map for the row bookkeeping and H = 1, W = M for the packed source
    ConvArgs a{xpk, wpk, nullptr, nullptr, nullptr, R, Cin, Cout_total, 1, M, out, rowidx, tile_co0};
    a.who = "gdm_gemm_grouped_hip";
    // 2 * CV_PANEL, below conv_lds_bytes(8): no packed output, so the waves' output tiles are never in LDS
    if (int refused = conv_launch<0, false, 1, true, 8, 8, MF_WAVES, false>(dim3(R / CV_PIX, 1), 2 * CV_PANEL, (hipStream_t)stream, a)) return refused;
    return gdm_launch_status("gemm_grouped_kernel");
}

// the 1x1 GEMM below with one weight set PER IMAGE (include/gdm.h: the split-K parts of the weight-gradient GEMM): H*W % 256 == 0
extern "C" int gdm_conv1x1_packed_wb_hip(const void* xpk, const void* wpk, long w_bstride, int B, int Cin, int Cout, int H, int W, float* out,
                                         void* stream)
{
    GDM_CHECK_ARG(xpk && wpk && out, "gdm_conv1x1_packed_wb_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && Cin >= 128 && Cin % 128 == 0 && Cout >= 1, "gdm_conv1x1_packed_wb_hip: Cin=%d Cout=%d (Cin a multiple of 128)", Cin, Cout);
    GDM_CHECK_ARG(W % 32 == 0 && H >= 1 && (H * W) % CV_PIX == 0, "gdm_conv1x1_packed_wb_hip: W=%d must be a multiple of 32 and H*W=%d of %d",
                  W, H * W, CV_PIX);
    GDM_CHECK_ARG(w_bstride >= 0 && w_bstride % 16 == 0, "gdm_conv1x1_packed_wb_hip: w_bstride=%ld", w_bstride);
    const long ptot = (long)B * H * W;
    const dim3 grid(gdm_cdiv(ptot, CV_PIX), gdm_cdiv(Cout, CV_CO));
    ConvArgs a{xpk, wpk, nullptr, nullptr, nullptr, B, Cin, Cout, H, W, out};
    a.wbstride = w_bstride; a.who = "gdm_conv1x1_packed_wb_hip";
    // no packed output: panels only
    if (int refused = conv_launch<0, false, 1, false, 8, 8, MF_WAVES, false>(grid, 2 * CV_PANEL, (hipStream_t)stream, a)) return refused;
    return gdm_launch_status("conv1x1_bf16x3_kernel (per-image weights)");
}

// 1x1 convolution / GEMM on the same kernel (one tap): out = act(scale * (W x) + shift), x packed by gdm_conv3x3_pack_act_hip.
// pixel_major != 0 writes out[B*H*W, Cout] (row per pixel) instead of NCHW.
static int conv1x1_launch(const void* xpk, const void* wpk, const float* scale, const float* shift,
                          int B, int Cin, int Cout, int H, int W, int stride, int act, int pixel_major, float* out, void* stream,
                          const char* who)
{
    GDM_CHECK_ARG(stride == 1 || stride == 2, "%s: stride=%d (1 or 2)", who, stride);
    GDM_CHECK_ARG(xpk && wpk && out, "%s: NULL pointer", who);
    GDM_CHECK_ARG(B >= 1 && cin_ok(Cin) && Cout >= 1, "%s: Cin=%d Cout=%d (Cin a multiple of 128, or 64)", who, Cin, Cout);
    GDM_CHECK_ARG(Cin != 64 || !pixel_major, "%s: Cin=64 is built for the NCHW output only", who);
    GDM_CHECK_ARG(W % 32 == 0 && H >= 1 && (H * W) % MF_WPIX == 0,
                  "%s: W=%d must be a multiple of 32 and H*W=%d of %d", who, W, H * W, MF_WPIX);
    GDM_CHECK_ARG(act == 0 || act == 1, "%s: act=%d", who, act);
    const long ptot = (long)B * H * W;
    const unsigned ptiles = gdm_cdiv(ptot, CV_PIX);
    hipStream_t s = (hipStream_t)stream;
    ConvArgs a{xpk, wpk, scale, shift, nullptr, B, Cin, Cout, H, W, out};
    a.stride = stride; a.who = who;
    int refused = 0;
    // 144-channel tiles (nine 16-channel blocks) where they divide Cout and fill the chip's rounds better than 128-channel ones: the
    // tap GEMMs of PSPUpsample have 9 * Cout' outputs -- 2304 at 64 pixel tiles = 1152 tiles of 128 (4.5 rounds of 256 CUs, paid as
    // 5) or 1024 tiles of 144 (4 rounds); 576 at 256 pixel tiles = 1280 tiles of 128, the last of every five half empty, or 1024 of 144
    if (Cin != 64 && !pixel_major && stride == 1 && Cout % 144 == 0) {
        const long r128 = gdm_cdiv((long)ptiles * gdm_cdiv(Cout, 128), 256) * 128, r144 = gdm_cdiv((long)ptiles * (Cout / 144), 256) * 144;
        if (r144 < r128) {
            const dim3 grid9(ptiles, Cout / 144);
            gdm_dispatch_int<2>(act, [&](auto A) {
                refused = conv_launch<decltype(A)::value, false, 1, false, 8, 9, MF_WAVES, false>(grid9, conv_lds_bytes(9), s, a);
            });
            if (refused) return refused;
            return gdm_launch_status("conv1x1_bf16x3_kernel (144-channel tiles)");
        }
    }
    const bool narrow = Cin != 64 && !pixel_major && narrow_tiles(ptiles, Cout);
    const unsigned ctiles = gdm_cdiv(Cout, narrow ? 64 : CV_CO);    // the last block's rows beyond Cout are zero weights, never stored
    // pixel tiles are the fast grid axis: workgroups that share a pixel tile land on one XCD.  (Channel tiles fastest was measured on the
    // 1024 -> 2304 tap GEMM in round 3: same time, 903 MB instead of 573 MB of fabric traffic -- each XCD then streams every weight panel.)
    const dim3 grid(ptiles, ctiles);
    // No packed output on this path, so the waves' output tiles are never in LDS: every launch below passes its two weight panels only,
    // which is below conv_lds_bytes(NCB) -- at 64-channel tiles 64 KiB, so that two workgroups share a CU.
    gdm_dispatch_int<2>(act, [&](auto A) {
        constexpr int ACT = decltype(A)::value;
        if (Cin == 64)                                              // one half-filled chunk: only its four non-zero k-steps are run
            refused = conv_launch<ACT, false, 1, false, 4, 8, MF_WAVES, false>(grid, 2 * CV_PANEL, s, a);
        else if (narrow)
            refused = conv_launch<ACT, false, 1, false, 8, 4, MF_WAVES, false>(grid, 2 * 64 * ROWB, s, a);
        else
            gdm_dispatch_bool(pixel_major != 0, [&](auto P) {
                refused = conv_launch<ACT, false, 1, decltype(P)::value, 8, 8, MF_WAVES, false>(grid, 2 * CV_PANEL, s, a);
            });
    });
    if (refused) return refused;
    return gdm_launch_status(narrow ? "conv1x1_bf16x3_kernel (64-channel tiles)" : "conv1x1_bf16x3_kernel");
}

extern "C" int gdm_conv1x1_packed_hip(const void* xpk, const void* wpk, const float* scale, const float* shift,
                                      int B, int Cin, int Cout, int H, int W, int act, int pixel_major, float* out, void* stream)
{
    return conv1x1_launch(xpk, wpk, scale, shift, B, Cin, Cout, H, W, 1, act, pixel_major, out, stream, "gdm_conv1x1_packed_hip");
}

// H, W = OUTPUT size; xpk = the (H stride) x (W stride) input (the downsample branch of a strided residual block reads every other pixel)
extern "C" int gdm_conv1x1_strided_hip(const void* xpk, const void* wpk, const float* scale, const float* shift,
                                       int B, int Cin, int Cout, int H, int W, int stride, int act, float* out, void* stream)
{
    return conv1x1_launch(xpk, wpk, scale, shift, B, Cin, Cout, H, W, stride, act, 0, out, stream, "gdm_conv1x1_strided_hip");
}

// The point-to-pixel fusion as ONE launch: the 1x1 GEMM above (stride 1, NCHW) whose epilogue adds the gathered point term and applies
// the folded BatchNorm and the activation (conv_mfma16_kernel, GADD) -- what gdm_conv1x1_strided_hip followed by
// gdm_gather_add_affine_act2_hip computes, bit for bit, without the fp32 map [B, Cout, H*W] written and read back between them.
// out (fp32 NCHW) and / or outpk (the packed operand of the next convolution / GEMM, as gdm_conv3x3_strided_hip writes it).
extern "C" int gdm_conv1x1_gather_add_hip(const void* xpk, const void* wpk, const int32_t* gidx, const float* gt, int gn, const float* scale,
                                          const float* shift, int B, int Cin, int Cout, int H, int W, int act, float* out, void* outpk,
                                          void* stream)
{
    const char* who = "gdm_conv1x1_gather_add_hip";
    GDM_CHECK_ARG(xpk && wpk && gidx && gt && scale && shift && (out || outpk), "%s: NULL pointer", who);
    GDM_CHECK_ARG(B >= 1 && cin_ok(Cin) && Cin != 64 && Cout >= 1, "%s: Cin=%d Cout=%d (Cin a multiple of 128)", who, Cin, Cout);
    GDM_CHECK_ARG(W >= 32 && W % 32 == 0 && H >= 1 && (H * W) % MF_WPIX == 0,
                  "%s: W=%d must be a multiple of 32 and H*W=%d of %d", who, W, H * W, MF_WPIX);
    GDM_CHECK_ARG(gn >= 1, "%s: gn=%d (the gathered term needs at least one column)", who, gn);
    GDM_CHECK_ARG(act == 0 || act == 1, "%s: act=%d (none or ReLU)", who, act);
    GDM_CHECK_ARG(!outpk || (Cout % 8 == 0 && ((long)B * H * W) % CV_PIX == 0),
                  "%s: packed output needs Cout %% 8 == 0 and B*H*W %% 256 == 0 (got Cout=%d, B*H*W=%ld)", who, Cout, (long)B * H * W);
    GDM_CHECK_ARG(((uintptr_t)gidx & 15) == 0, "%s: gidx must be 16-byte aligned (the epilogue loads four indices at once)", who);
    const long ptot = (long)B * H * W;
    const unsigned ptiles = gdm_cdiv(ptot, CV_PIX);
    const bool narrow = narrow_tiles(ptiles, Cout);                 // the tile width conv1x1_launch takes for this shape
    const dim3 grid(ptiles, gdm_cdiv(Cout, narrow ? 64 : CV_CO));
    // weight panels, or (packed output) the waves' output tiles where those are larger
    const int tiles = conv_lds_bytes(narrow ? 4 : 8);
    // behind them the workgroup's rows of gt, gn + 1 floats apart (conflict-free across the 16 channels of a fragment), where a workgroup
    // lies inside one image and the rows fit the CU's 160 KiB; 64-channel tiles stay at two workgroups per CU unless the grid has no
    // second workgroup for a CU anyway.  Otherwise the lanes gather from global memory.
    const long trows = (long)(narrow ? 64 : CV_CO) * (gn + 1) * 4;
    const long smem = tiles + trows;
    const bool stage_t = (H * W) % CV_PIX == 0 && smem <= (narrow && (long)grid.x * grid.y > 256 ? LDS_MAX / 2 : LDS_MAX);
    ConvArgs a{xpk, wpk, scale, shift, nullptr, B, Cin, Cout, H, W, out};
    a.outpk = outpk; a.gidx = gidx; a.gt = gt; a.gn = gn; a.gt_lds = stage_t ? tiles : 0; a.who = who;
    const int SM = stage_t ? (int)smem : tiles;
    int refused = 0;                                                // packed operands of 2 GiB or more
    gdm_dispatch_int<2>(act, [&](auto A) {
        gdm_dispatch_bool(narrow, [&](auto N4) {
            refused = conv_launch<decltype(A)::value, false, 1, false, 8, decltype(N4)::value ? 4 : 8, MF_WAVES, true>(grid, SM, (hipStream_t)stream, a);
        });
    });
    if (refused) return refused;
    return gdm_launch_status(narrow ? "conv1x1_gather_add_kernel (64-channel tiles)" : "conv1x1_gather_add_kernel");
}
