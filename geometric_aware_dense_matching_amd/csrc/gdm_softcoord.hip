// Differentiable soft assignment WITHOUT the similarity matrix, gfx950: the training half of the soft matching of gdm_match.hip
// (DESIGN.md 6k / 6l).  Per scene row r (unit descriptor x_r) over the M model vertices (unit descriptors y_c, coordinates xyz_c),
// s_rc = <x_r, y_c> in split-bf16 with fp32 accumulation, temperature gamma:
//   Z_r    = sum_c exp(gamma (s_rc - 1))                    fixed shift 1 (cosines are <= 1), 0 < gamma <= 40: no running maximum
//   lse_r  = gamma + log Z_r
//   soft_r = sum_c exp(gamma (s_rc - 1)) xyz_c / Z_r        the expected model coordinate
// over exactly the M real columns (there is no padding column here).  Backward, with upstream a_r = dL/dlse_r, b_r = dL/dsoft_r,
// p_rc = exp(gamma s_rc - lse_r) and k_r = a_r - b_r . soft_r:
//   G_rc = dL/ds_rc = gamma p_rc (k_r + b_r . xyz_c)        gx_r = sum_c G_rc y_c        gy_c = sum_r G_rc x_r
// Nothing of size [R, M] touches HBM: the S tile is recomputed in both backward kernels, flash-attention style.
//
// One kernel template, three modes, in the owner / stream structure of circle_mm_kernel (gdm_circle.hip), whose operands -- the
// buffers gdm_circle_match_pack_hip writes -- it reads: 128 owner items per workgroup, 32 per wave, whole K = 128 in registers as
// split-bf16 fragments; the other side is streamed through LDS in 64-item stages.
//   MODE 0  forward   owner = scene rows, stream = vertices: S tile (24 MFMAs) -> w = exp2(fma(s, k2, -k2)), Z / Sx / Sy / Sz per lane
//   MODE 1  grad x    owner = scene rows, stream = vertices: S tile again, G in the accumulator layout, fed STRAIGHT to the second
//                     MFMA as its B operand (gX^T[d, r] += Y^T[d, c] G[c, r]): the k-order of the d-major copy of cm_pack_kernel
//   MODE 2  grad y    owner = vertices, stream = a slice of the scene rows per workgroup; partial sums [P][Mp,128], added in
//                     ascending P by sc_sum_parts_kernel.  No float atomics anywhere: two runs are bit-identical.
// Masks: a padded column (c >= M, a zero row) has s = 0 and would weigh exp(-gamma), so every mode drops it explicitly; a padded
// row (r >= R) carries lse = k = b = 0 whatever the caller's buffers hold (the loads are guarded), so it adds exactly 0 to gy.
// The skeleton's tile code -- operand load, stage fills, second product, output store -- is gdm_owner_stream.h, shared with
// circle_mm_kernel (profiles/tile_helpers.md: the instructions it changed here, and that it cost no time).
#include "gdm_owner_stream.h"
#include <math.h>

namespace {

constexpr int LDS_SIDE = OS_ST * 5 * (int)sizeof(float);     // per streamed item: xyz (MODE 0 / 1) or k, b, -lse log2 e (MODE 2)
constexpr float LOG2E = 1.4426950408889634f;

#define SC_V3(a) "+v"((a)[0]), "+v"((a)[1]), "+v"((a)[2])
#define SC_V5(a) "+v"((a)[0]), "+v"((a)[1]), "+v"((a)[2]), "+v"((a)[3]), "+v"((a)[4])

struct ScArgs {
    const unsigned char* xrows;     // scene rows, packed [Rp]
    const unsigned char* xtp;       // scene d-major tiles
    const unsigned char* yrows;     // vertex rows, packed [Mp]
    const unsigned char* ytp;
    const float* xyz;               // [M,3]
    float* lse;                     // [R]    forward out / backward in
    float* soft;                    // [R,3]  forward out
    const float* kb;                // [R,4]  backward: k_r, b_r
    float* gout;                    // MODE 1: gX [R,128]; MODE 2: partial gY [P][Mp,128]
    int R, Rp, M, Mp, P;
    float gamma, k2;                // k2 = gamma log2(e)
};

template <int MODE>
__global__ __launch_bounds__(OS_THREADS, 2) void soft_coord_kernel(const ScArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* lrows = smem;
    float* lside = reinterpret_cast<float*>(smem + LDS_ROWS);                   // [OS_ST][3] (MODE 0 / 1) or [OS_ST][5] (MODE 2)
    unsigned char* ltp = smem + LDS_ROWS + LDS_SIDE;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    constexpr bool own_is_x = MODE != 2;
    const int nown_blocks = (own_is_x ? a.Rp : a.Mp) / OS_OWN;
    const int ob = blockIdx.x % nown_blocks;            // owner block
    const int part = blockIdx.x / nown_blocks;          // MODE 2: slice of the stream
    const int own0 = ob * OS_OWN + wave * 32;           // this wave's first owner item
    const unsigned char* orows = own_is_x ? a.xrows : a.yrows;
    const unsigned char* srows = own_is_x ? a.yrows : a.xrows;
    const unsigned char* stp = own_is_x ? a.ytp : a.xtp;
    const int nstage = (own_is_x ? a.Mp : a.Rp) / OS_ST;

    // owner operand: 8 k-steps x (hi, lo)
    gdm_u32x4 ohi[8], olo[8];
    os_load_owner(orows, own0 + j, h, ohi, olo);
    // per-lane constants of the owner item
    const int own = own0 + j;
    const bool own_ok = own < (own_is_x ? a.R : a.M);
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, onl = 0.f;    // MODE 1: k, b, -lse log2 e of the row; MODE 2: xyz of the vertex
    if (MODE == 1 && own_ok) {
        const float4 v = *reinterpret_cast<const float4*>(a.kb + (long)own * 4);
        o0 = v.x; o1 = v.y; o2 = v.z; o3 = v.w;
        onl = -a.lse[own] * LOG2E;
    }
    if (MODE == 2 && own_ok) {
        o1 = a.xyz[3 * (long)own]; o2 = a.xyz[3 * (long)own + 1]; o3 = a.xyz[3 * (long)own + 2];
    }
    const float k2 = a.k2, gam = a.gamma;
    float Z = 0.f, Sx = 0.f, Sy = 0.f, Sz = 0.f;

    gdm_f32x16 outacc[4];
    if (MODE != 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) outacc[c][i] = 0.f;
    }

    for (int st = (MODE == 2 ? part : 0); st < nstage; st += (MODE == 2 ? a.P : 1)) {
        __syncthreads();                                            // the previous stage's readers are done
        {
            os_fill_rows(srows, st, lrows, tid);
            if (MODE != 0) os_fill_tp(stp, st, ltp, tid);
            if (MODE != 2) {                                        // the stage's xyz (768 B), zero for a padded column
                if (tid < OS_ST * 3) {
                    const long e = (long)st * OS_ST * 3 + tid;
                    lside[tid] = e < (long)a.M * 3 ? a.xyz[e] : 0.f;
                }
            } else if (tid < OS_ST) {                               // per streamed scene row: k, b, -lse log2 e; zero for a padded row
                const long r = (long)st * OS_ST + tid;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                float nl = 0.f;
                if (r < a.R) {
                    v = *reinterpret_cast<const float4*>(a.kb + r * 4);
                    nl = -a.lse[r] * LOG2E;
                }
                lside[tid * 5] = v.x; lside[tid * 5 + 1] = v.y; lside[tid * 5 + 2] = v.z; lside[tid * 5 + 3] = v.w;
                lside[tid * 5 + 4] = nl;
            }
        }
        __syncthreads();

#pragma unroll 1
        for (int sub = 0; sub < OS_ST / 32; ++sub) {
            const int t32 = st * (OS_ST / 32) + sub;                // index of this 32-item sub-tile in the stream
            // ---- S tile: acc[i][j] = <stream_i, owner_j> ----  os_s_tile restated: through the helper soft_coord_kernel<0> and <1>
            // came out 1 to 3 % slower at R = 49152, M = 4096 (profiles/tile_helpers.md, section 3)
            gdm_f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const gdm_bf16x8 sh = __builtin_bit_cast(gdm_bf16x8, *reinterpret_cast<const gdm_u32x4*>(lrows + gdm_swz<ROWB>(sub * 32 + j, 2 * s + h)));
                const gdm_bf16x8 sl = __builtin_bit_cast(gdm_bf16x8, *reinterpret_cast<const gdm_u32x4*>(lrows + gdm_swz<ROWB>(sub * 32 + j, 16 + 2 * s + h)));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sh, __builtin_bit_cast(gdm_bf16x8, olo[s]), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sl, __builtin_bit_cast(gdm_bf16x8, ohi[s]), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sh, __builtin_bit_cast(gdm_bf16x8, ohi[s]), acc, 0, 0, 0);
            }
            // ---- element-wise: register r <-> streamed item i = acc_row(r >> 3, h, r & 7), lane <-> owner item j ----
            const int cbase = t32 * 32;                             // MODE 0 / 1: first vertex of the sub-tile
            float G[16];
            if (MODE != 2) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    float xv[8][3];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int i = sub * 32 + acc_row(ks, h, q);
                        xv[q][0] = lside[i * 3]; xv[q][1] = lside[i * 3 + 1]; xv[q][2] = lside[i * 3 + 2];
                    }
                    GDM_SETTLE_LDS(SC_V3(xv[0]), SC_V3(xv[1]), SC_V3(xv[2]), SC_V3(xv[3]), SC_V3(xv[4]), SC_V3(xv[5]), SC_V3(xv[6]), SC_V3(xv[7]));
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const bool valid = cbase + acc_row(ks, h, q) < a.M;       // a padded column weighs nothing
                        const float s = acc[8 * ks + q];
                        if (MODE == 0) {
                            const float w = valid ? __builtin_amdgcn_exp2f(__builtin_fmaf(s, k2, -k2)) : 0.f;
                            Z += w;
                            Sx = __builtin_fmaf(w, xv[q][0], Sx);
                            Sy = __builtin_fmaf(w, xv[q][1], Sy);
                            Sz = __builtin_fmaf(w, xv[q][2], Sz);
                        } else {
                            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s, k2, onl));
                            const float t = __builtin_fmaf(o3, xv[q][2], __builtin_fmaf(o2, xv[q][1], __builtin_fmaf(o1, xv[q][0], o0)));
                            G[8 * ks + q] = (valid && own_ok) ? gam * p * t : 0.f;
                        }
                    }
                }
            } else {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    float rd[4][5];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int i = sub * 32 + acc_row(g4 >> 1, h, (g4 & 1) * 4 + q);
#pragma unroll
                        for (int e = 0; e < 5; ++e) rd[q][e] = lside[i * 5 + e];
                    }
                    GDM_SETTLE_LDS(SC_V5(rd[0]), SC_V5(rd[1]), SC_V5(rd[2]), SC_V5(rd[3]));
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float s = acc[4 * g4 + q];
                        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s, k2, rd[q][4]));
                        const float t = __builtin_fmaf(rd[q][3], o3, __builtin_fmaf(rd[q][2], o2, __builtin_fmaf(rd[q][1], o1, rd[q][0])));
                        G[4 * g4 + q] = own_ok ? gam * p * t : 0.f;   // a padded vertex gets no gradient; a padded row has k = b = 0: t = 0
                    }
                }
            }
            if (MODE == 0) continue;
            os_second_product(ltp, sub, j, h, G, outacc);
        }
    }

    if (MODE == 0) {
        // lanes j and j + 32 hold the two halves of row j's columns: one fixed-order addition each
        float pz = __shfl_xor(Z, 32, 64), px = __shfl_xor(Sx, 32, 64), py = __shfl_xor(Sy, 32, 64), pw = __shfl_xor(Sz, 32, 64);
        GDM_SETTLE_LDS("+v"(pz), "+v"(px), "+v"(py), "+v"(pw));
        Z += pz; Sx += px; Sy += py; Sz += pw;
        if (h == 0 && own_ok) {
            // the logarithm and the divisions in fp64, as soft_merge_kernel evaluates them: they add nothing to the fp32 sums' error
            const double z = (double)Z;
            a.lse[own] = (float)((double)gam + log(z));
            a.soft[3 * (long)own] = (float)((double)Sx / z);
            a.soft[3 * (long)own + 1] = (float)((double)Sy / z);
            a.soft[3 * (long)own + 2] = (float)((double)Sz / z);
        }
        return;
    }
    // ---- MODE 1 / 2: outacc[db][r] = grad[owner j][d = db*32 + acc_row(r)] ----
    if (MODE == 1 && !own_ok) return;                               // gX has R rows; gY partials keep their Mp rows (zeros beyond M)
    float* ob_out = a.gout + (MODE == 2 ? (long)part * a.Mp * 128 : 0L) + (long)own * 128;
    os_store_out<false>(ob_out, h, outacc);
}

// gy[c][d] = sum over p = 0 .. P-1, in that order, of part[p][c][d]   (c < M; n4 = M * 32 float4 per part, stride4 = Mp * 32)
__global__ __launch_bounds__(256) void sc_sum_parts_kernel(const float4* __restrict__ part, int P, long n4, long stride4, float4* __restrict__ gy)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 s = part[i];
    for (int p = 1; p < P; ++p) {
        const float4 o = part[(long)p * stride4 + i];
        s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
    }
    gy[i] = s;
}

template <int MODE>
int launch_mode(const ScArgs& a, hipStream_t stream)
{
    constexpr int lds = LDS_ROWS + LDS_SIDE + (MODE != 0 ? LDS_TP : 0);
    const int grid = MODE == 2 ? (a.Mp / OS_OWN) * a.P : a.Rp / OS_OWN;
    gdm_allow_lds<soft_coord_kernel<MODE>>(lds);
    hipLaunchKernelGGL((soft_coord_kernel<MODE>), dim3(grid), dim3(OS_THREADS), lds, stream, a);
    return gdm_launch_status("soft_coord_kernel");
}

int fill_args(ScArgs& a, const void* xrows, const void* xtp, const void* yrows, const void* ytp, const float* xyz, int R, int M, float gamma,
              const char* who)
{
    GDM_CHECK_ARG(xrows && xtp && yrows && ytp && xyz, "%s: NULL pointer", who);
    GDM_CHECK_ARG(R >= 1 && M >= 1, "%s: R=%d M=%d", who, R, M);
    GDM_CHECK_ARG(R <= (1 << 30) && M <= (1 << 30), "%s: R=%d M=%d beyond 2^30", who, R, M);
    GDM_CHECK_ARG(gamma > 0.f && gamma <= GDM_SOFT_COORD_MAX_GAMMA, "%s: gamma=%g outside (0, %g]", who, (double)gamma, (double)GDM_SOFT_COORD_MAX_GAMMA);
    GDM_CHECK_ARG((((uintptr_t)xrows | (uintptr_t)xtp | (uintptr_t)yrows | (uintptr_t)ytp) & 15) == 0, "%s: the packed rows must be 16-byte aligned", who);
    a.xrows = (const unsigned char*)xrows; a.xtp = (const unsigned char*)xtp;
    a.yrows = (const unsigned char*)yrows; a.ytp = (const unsigned char*)ytp;
    a.xyz = xyz;
    a.lse = nullptr; a.soft = nullptr; a.kb = nullptr; a.gout = nullptr;
    a.R = R; a.Rp = (R + 127) / 128 * 128; a.M = M; a.Mp = (M + 127) / 128 * 128; a.P = 1;
    a.gamma = gamma; a.k2 = gamma * LOG2E;
    return 0;
}

} // namespace

extern "C" int gdm_soft_coord_bwd_parts(int R, int M)
{
    return os_bwd_parts(R, M);
}

extern "C" int gdm_soft_coord_fwd_hip(const void* xrows, const void* xtp, const void* yrows, const void* ytp, const float* xyz, int R, int M,
                                      float gamma, float* lse, float* soft, void* stream)
{
    ScArgs a;
    int rc = fill_args(a, xrows, xtp, yrows, ytp, xyz, R, M, gamma, "gdm_soft_coord_fwd_hip");
    if (rc) return rc;
    GDM_CHECK_ARG(lse && soft, "gdm_soft_coord_fwd_hip: NULL output");
    a.lse = lse; a.soft = soft;
    return launch_mode<0>(a, (hipStream_t)stream);
}

extern "C" int gdm_soft_coord_bwd_hip(const void* xrows, const void* xtp, const void* yrows, const void* ytp, const float* xyz, int R, int M,
                                      float gamma, const float* lse, const float* kb, float* gx, float* gy_part, float* gy, void* stream)
{
    ScArgs a;
    int rc = fill_args(a, xrows, xtp, yrows, ytp, xyz, R, M, gamma, "gdm_soft_coord_bwd_hip");
    if (rc) return rc;
    GDM_CHECK_ARG(lse && kb && (gx || gy), "gdm_soft_coord_bwd_hip: NULL pointer");
    GDM_CHECK_ARG(!gy || gy_part, "gdm_soft_coord_bwd_hip: gy needs the gy_part workspace");
    GDM_CHECK_ARG((((uintptr_t)kb | (uintptr_t)gy_part | (uintptr_t)gy) & 15) == 0, "gdm_soft_coord_bwd_hip: kb, gy_part and gy must be 16-byte aligned");
    a.lse = const_cast<float*>(lse); a.kb = kb;
    if (gx) {                                                       // either gradient may be left out (NULL): its launches are skipped
        a.gout = gx;
        if ((rc = launch_mode<1>(a, (hipStream_t)stream))) return rc;
    }
    if (!gy) return 0;
    a.gout = gy_part;
    a.P = gdm_soft_coord_bwd_parts(R, M);
    if ((rc = launch_mode<2>(a, (hipStream_t)stream))) return rc;
    const long n4 = (long)M * 32;
    hipLaunchKernelGGL(sc_sum_parts_kernel, dim3(gdm_cdiv(n4, 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(gy_part), a.P,
                       n4, (long)a.Mp * 32, reinterpret_cast<float4*>(gy));
    return gdm_launch_status("sc_sum_parts_kernel");
}
