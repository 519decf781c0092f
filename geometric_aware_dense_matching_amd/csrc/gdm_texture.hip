// Texture pyramids on the device, gfx950 (gdm_texture_mips_hip; texture.build_mips_numpy restates it bit for bit): an
// image u8[H,W,3] becomes level 0 of a pyramid of dword texels (r, g, b, 0), and every further level is made from the one before it by
// THE TEXTURE RULE of include/gdm.h, whose layout is in gdm_texture.h.
//   pack_kernel   one thread per texel of level 0: three byte loads, one dword store.
//   mip_kernel    one thread per texel of level l: four dword loads from level l - 1 (indices clamped to it), (a + b + c + d + 2) >> 2
//                 per channel, one dword store.  One launch per level: level l reads what the launch before it wrote, and the order
//                 comes from the stream alone.
// No memset node, no allocation and no host read: the entry captures in a hipGraph.
#include "gdm_texture.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void pack_kernel(const uint8_t* __restrict__ image, long count, uint32_t* __restrict__ pyr)
{
    const long t0 = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
    for (long i = t0; i < count; i += step)
        pyr[i] = (uint32_t)image[i * 3] | ((uint32_t)image[i * 3 + 1] << 8) | ((uint32_t)image[i * 3 + 2] << 16);
}

__global__ __launch_bounds__(kThreads) void mip_kernel(const uint32_t* __restrict__ src, int Ws, int Hs, uint32_t* __restrict__ dst, int Wd,
                                                       int Hd)
{
    const long count = (long)Wd * Hd;
    const long t0 = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
    for (long i = t0; i < count; i += step) {
        const int x = (int)(i % Wd), y = (int)(i / Wd);
        const int xa = min(2 * x, Ws - 1), xb = min(2 * x + 1, Ws - 1), ya = min(2 * y, Hs - 1), yb = min(2 * y + 1, Hs - 1);
        const uint32_t a = src[(long)ya * Ws + xa], b = src[(long)ya * Ws + xb], c = src[(long)yb * Ws + xa], d = src[(long)yb * Ws + xb];
        uint32_t out = 0;
#pragma unroll
        for (int sh = 0; sh < 24; sh += 8)
            out |= ((((a >> sh) & 255u) + ((b >> sh) & 255u) + ((c >> sh) & 255u) + ((d >> sh) & 255u) + 2u) >> 2) << sh;
        dst[i] = out;
    }
}

int grid_for(long count) { return (int)(gdm_cdiv(count, kThreads) < 4096 ? gdm_cdiv(count, kThreads) : 4096); }

} // namespace

extern "C" long gdm_texture_pyramid_texels(int H, int W, int L)
{
    if (H < 1 || H > kTexMaxSide || W < 1 || W > kTexMaxSide || L < 1 || L > tex_full_levels(W, H)) return 0;
    return tex_level_offset(W, H, L);
}

extern "C" int gdm_texture_mips_hip(const uint8_t* image, int H, int W, int L, void* pyr, long pyr_texels, void* stream)
{
    GDM_CHECK_ARG(image && pyr, "gdm_texture_mips_hip: NULL pointer");
    GDM_CHECK_ARG(H >= 1 && H <= kTexMaxSide && W >= 1 && W <= kTexMaxSide, "gdm_texture_mips_hip: H=%d W=%d not in [1, %d]", H, W,
                  kTexMaxSide);
    GDM_CHECK_ARG(L >= 1 && L <= tex_full_levels(W, H), "gdm_texture_mips_hip: L=%d not in [1, %d] for a %d x %d image", L,
                  tex_full_levels(W, H), W, H);
    const long need = tex_level_offset(W, H, L);
    GDM_CHECK_ARG(pyr_texels >= need && pyr_texels < (1l << 31), "gdm_texture_mips_hip: pyramid of %ld texels, %ld needed (below 2^31)",
                  pyr_texels, need);
    GDM_CHECK_ARG(((uintptr_t)pyr & 3) == 0, "gdm_texture_mips_hip: pyr must be 4-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    uint32_t* base = (uint32_t*)pyr;
    hipLaunchKernelGGL(pack_kernel, dim3(grid_for((long)H * W)), dim3(kThreads), 0, s, image, (long)H * W, base);
    int rc = gdm_launch_status("pack_kernel");
    for (int l = 1; l < L && !rc; ++l) {
        const int Ws = tex_level_side(W, l - 1), Hs = tex_level_side(H, l - 1), Wd = tex_level_side(W, l), Hd = tex_level_side(H, l);
        hipLaunchKernelGGL(mip_kernel, dim3(grid_for((long)Wd * Hd)), dim3(kThreads), 0, s, base + tex_level_offset(W, H, l - 1), Ws, Hs,
                           base + tex_level_offset(W, H, l), Wd, Hd);
        rc = gdm_launch_status("mip_kernel");
    }
    return rc;
}
