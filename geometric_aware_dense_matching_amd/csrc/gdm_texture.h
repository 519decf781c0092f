// The one copy of THE TEXTURE RULE of include/gdm.h (gdm_texture_mips_hip; texture.py restates it in numpy bit for
// bit), shared by the mip builder of gdm_texture.hip, the textured resolve of gdm_render.hip and the textured surface sampler of
// gdm_modelprep.hip: the pyramid's layout, the validation of an object's table row, the level choice without a transcendental and
// the bilinear fetch with 8-bit fractions and an integer blend.  A texel is one dword, (r, g, b, 0) from the low byte up.
#pragma once
#include "gdm_common.h"

constexpr int kTexMaxSide = 16384;
constexpr int kTexMaxLevels = 15;                                          // 1 + floor(log2(16384))

struct TexObj { long off; int W0, H0, L; };                                // a validated table row; W0 == 0: no texture

__host__ __device__ __forceinline__ int tex_level_side(int side0, int l) { return (side0 >> l) > 1 ? (side0 >> l) : 1; }

// 1 + floor(log2(max(W0, H0))): the level whose larger side is 1
__host__ __device__ __forceinline__ int tex_full_levels(int W0, int H0)
{
    int m = W0 > H0 ? W0 : H0, l = 1;
    while (m > 1) { m >>= 1; ++l; }
    return l;
}

// Texels of levels 0 .. l-1: where level l starts.  The caller has checked the sides and l.
__host__ __device__ __forceinline__ long tex_level_offset(int W0, int H0, int l)
{
    long t = 0;
    for (int k = 0; k < l; ++k) t += (long)tex_level_side(W0, k) * tex_level_side(H0, k);
    return t;
}

// A row (offset, W0, H0, L) of a table the host cannot look at: true, and `t` filled, only when every texel of the pyramid lies inside
// the buffer of tex_texels texels.  Everything else, W0 == 0 included, is "no texture".
__host__ __device__ __forceinline__ bool tex_row_valid(long long off, long long W0, long long H0, long long L, long tex_texels, TexObj& t)
{
    t.off = 0; t.W0 = 0; t.H0 = 0; t.L = 0;
    if (!(W0 >= 1 && W0 <= kTexMaxSide && H0 >= 1 && H0 <= kTexMaxSide)) return false;
    if (!(L >= 1 && L <= tex_full_levels((int)W0, (int)H0))) return false;
    if (!(off >= 0 && off <= (long long)tex_texels)) return false;
    if (tex_level_offset((int)W0, (int)H0, (int)L) > (long long)tex_texels - off) return false;
    t.off = (long)off; t.W0 = (int)W0; t.H0 = (int)H0; t.L = (int)L;
    return true;
}

#ifdef __HIPCC__
// The smallest l with rho2 <= 4^l, capped at L - 1; a NaN goes to the coarsest level.
__device__ __forceinline__ int tex_level(double rho2, int L)
{
    int l = 0;
    double t = 1.0;
    while (l < L - 1 && !(rho2 <= t)) { ++l; t *= 4.0; }
    return l;
}

// One axis of the fetch: the two clamped texel indices and the 8-bit fraction of coordinate c (in [0, 1] inside the image) on a level
// of n texels.
__device__ __forceinline__ void tex_axis(double c, int n, int& i0, int& i1, int& fr)
{
    const double x = c * (double)n - 0.5;
    const double x0 = floor(x);
    fr = (int)floor((x - x0) * 256.0);
    const int b = (int)fmin(fmax(x0, -1.0), (double)n);                    // before the conversion: x0 may exceed an int
    i0 = min(max(b, 0), n - 1);
    i1 = min(max(b + 1, 0), n - 1);
}

// Fetch(level, u, v): the blended texel, packed like a stored one.
__device__ __forceinline__ uint32_t tex_fetch(const uint32_t* __restrict__ tex, const TexObj& t, int level, double u, double v, int flip_v)
{
    const int Wl = tex_level_side(t.W0, level), Hl = tex_level_side(t.H0, level);
    const uint32_t* lv = tex + t.off + tex_level_offset(t.W0, t.H0, level);
    if (!(fabs(u) <= 1.7976931348623157e308) || !(fabs(v) <= 1.7976931348623157e308)) return lv[0];
    int x0, x1, fx, y0, y1, fy;
    tex_axis(u, Wl, x0, x1, fx);
    tex_axis(flip_v ? 1.0 - v : v, Hl, y0, y1, fy);
    const uint32_t c00 = lv[(long)y0 * Wl + x0], c10 = lv[(long)y0 * Wl + x1], c01 = lv[(long)y1 * Wl + x0], c11 = lv[(long)y1 * Wl + x1];
    uint32_t out = 0;
#pragma unroll
    for (int sh = 0; sh < 24; sh += 8) {
        const int a = (int)((c00 >> sh) & 255u), b = (int)((c10 >> sh) & 255u), c = (int)((c01 >> sh) & 255u), d = (int)((c11 >> sh) & 255u);
        const int top = a * (256 - fx) + b * fx, bot = c * (256 - fx) + d * fx;
        out |= (uint32_t)((top * (256 - fy) + bot * fy + 32768) >> 16) << sh;
    }
    return out;
}
#endif
