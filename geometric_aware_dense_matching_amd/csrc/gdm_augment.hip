// Front end on the device, gfx950: the YCB-V training item's colour, noise and background augmentation of the crop
// (datasets/ycbv/ycbv_pbr.py:317-386, :468-477) by the integer rule of include/gdm.h (gdm_augment_crops_hip), and the box jitter with
// counter-based draws (gdm_dzi_boxes_hip).
//   augment_pass_kernel<0>   levels from the normalised crop, pass 0 of rgb_add_noise, the uint8 image into the workspace
//   augment_pass_kernel<1>   add_real_back while the tile is loaded, pass 1 where the crop drew one, normalize_color, the depth paste
// One workgroup per (crop, 32 x 32 tile).  The stencil chain of a pass (sharpen -> motion blur -> Gaussian blur) is data-dependent from
// stage to stage, so the workgroup keeps the tile plus the chain's cumulative halo in LDS, one packed r | g << 8 | b << 16 dword per
// pixel, and the stages ping-pong between two such buffers; halo pixels are recomputed, never exchanged.  The halo is the sum of the
// reaches of the stages THIS crop drew (sharpen 1, motion blur the largest tap offset <= 15, Gaussian 1 or 2): four crops in five
// draw none and load the bare tile.  Stage k writes the tile extended by the reach of the stages after it, clipped to the image; a
// tap is reflected in IMAGE coordinates (REFLECT_101) before the LDS origin is subtracted, and with S >= 32 the reflected pixel lies
// inside the same extended tile (it is at most `reach` pixels from the border the tile touches).
// LDS layout: a dword per pixel makes every tap one ds_read_b32 for all three channels; the lanes of a 32-lane group walk a row, i.e.
// consecutive banks, and the row pitch of 69 dwords (odd) keeps the lanes that wrap into the next row off the banks of the row's end.
// The gain of step 1 is folded into the tile load, the noise and the normalisation into the store.  Every block derives its crop's
// draws itself (thirty hash words and a Bresenham line of at most 16 points, by one thread): no parameter buffer, no extra launch.
#include "gdm_common.h"
#define GDM_AUG_TABLE static __constant__ const
#include "gdm_augment_tables.h"

namespace {

constexpr int kTile = 32;
constexpr int kMaxHalo = 18;                                               // sharpen 1 + motion 15 + Gaussian 2
constexpr int kExt = kTile + 2 * kMaxHalo;                                 // 68
constexpr int kPitch = kExt + 1;                                           // 69 dwords
constexpr int kThreads = 256;
constexpr uint32_t kP20 = 0xccccccccu, kP80 = 0x33333333u;                 // word > kP20: probability 0.2; word > kP80: probability 0.8

__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t below(uint32_t w, uint32_t n) { return (uint32_t)(((unsigned long long)w * n) >> 32); }

struct PassParams {
    int active;                                                            // 0: the load is followed by the store at once
    int ks, kv;
    int sharpen, sh_c, sh_q;
    int motion, n_taps, reach_m;
    int tap_dy[16], tap_dx[16];
    int gauss_r, gw[3];
    int sigma, extra;
    uint32_t hs0, hs1;
    int bank, wy, wx;                                                      // the window of the paste (pass 1)
};

// The draws of pass q of crop hash hb (include/gdm.h), by one thread.
__device__ void draw_pass(uint32_t hb, int q, int force, PassParams& p)
{
    const uint32_t k0 = 16u * (uint32_t)q;
    auto D = [&](uint32_t j) { return mix32(hb ^ (k0 + j)); };
    p.ks = 320 + (int)below(D(0), 52);
    p.kv = 294 + (int)below(D(1), 52);
    p.sharpen = force || D(2) > kP20;
    const int u = (int)(D(3) >> 24);
    p.sh_c = 2304 + 3 * u;
    p.sh_q = 256 + 3 * u;
    p.motion = force || D(4) > kP20;
    p.n_taps = 0;
    p.reach_m = 0;
    if (p.motion) {
        const int angle = (int)below(D(5), 360), L = (int)below(D(6), 15) + 1;
        const int cs = gdm_aug_cos_q14[angle], sn = gdm_aug_cos_q14[(angle + 270) % 360];
        const int ac = cs < 0 ? -cs : cs, as = sn < 0 ? -sn : sn;
        const int a = ((ac > as ? ac : as) * L * 2) >> 14;
        if (a <= 0) {
            p.motion = 0;
        } else {
            const int cx = a / 2, ex = cx + cs * L / 16384, ey = cx + sn * L / 16384;      // C division truncates towards zero
            const int dx = ex > cx ? ex - cx : cx - ex, sx = ex > cx ? 1 : -1;
            const int dy = -(ey > cx ? ey - cx : cx - ey), sy = ey > cx ? 1 : -1;
            int err = dx + dy, x = cx, y = cx, n = 0, reach = 0;
            for (int it = 0; it < 32; ++it) {                              // the line has at most 16 points
                if (x >= 0 && x < a && y >= 0 && y < a && n < 16) {
                    p.tap_dy[n] = y - cx;
                    p.tap_dx[n] = x - cx;
                    const int ry = y > cx ? y - cx : cx - y, rx = x > cx ? x - cx : cx - x;
                    reach = reach > ry ? reach : ry;
                    reach = reach > rx ? reach : rx;
                    ++n;
                }
                if (x == ex && y == ey) break;
                const int e2 = 2 * err;
                if (e2 >= dy) { err += dy; x += sx; }
                if (e2 <= dx) { err += dx; y += sy; }
            }
            p.n_taps = n;                                                  // >= 1: the centre lies inside the kernel
            p.reach_m = reach > 15 ? 15 : reach;                           // <= L <= 15 by construction
        }
    }
    p.gauss_r = 0;
    if (force || D(7) > kP20) {
        const int five = !(D(8) > kP80), l = (int)(D(9) >> 24);
        p.gauss_r = five ? 2 : 1;
        p.gw[0] = five ? gdm_aug_gauss5[l][0] : gdm_aug_gauss3[l][0];
        p.gw[1] = five ? gdm_aug_gauss5[l][1] : gdm_aug_gauss3[l][1];
        p.gw[2] = five ? gdm_aug_gauss5[l][2] : 0;
    }
    p.sigma = (int)below(D(11), D(10) > kP80 ? 15u : 25u);
    p.extra = D(12) > kP20;
    p.hs0 = mix32(hb ^ (256u + 2u * (uint32_t)q));
    p.hs1 = mix32(hb ^ (256u + 2u * (uint32_t)q + 1u));
}

__device__ __forceinline__ int reflect101(int i, int S) { return i < 0 ? -i : (i >= S ? 2 * S - 2 - i : i); }

// Step 1, the saturation / value gain on max and min.
__device__ __forceinline__ uint32_t hsv_gain(int r, int g, int b, int ks, int kv)
{
    const int M = max(r, max(g, b)), m = min(r, min(g, b)), d = M - m;
    const int M2 = min(255, (M * kv) >> 8);
    if (d == 0) return (uint32_t)M2 * 0x010101u;
    const int s = (255 * d + (M >> 1)) / M;
    const int s2 = min(255, (s * ks) >> 8);
    const int m2 = M2 - (M2 * s2 + 127) / 255;
    const int R = M2 - m2, h = d >> 1;
    const int r2 = m2 + ((r - m) * R + h) / d, g2 = m2 + ((g - m) * R + h) / d, b2 = m2 + ((b - m) * R + h) / d;
    return (uint32_t)r2 | ((uint32_t)g2 << 8) | ((uint32_t)b2 << 16);
}

__device__ __forceinline__ int noise_of(uint32_t w, int sigma)
{
    const int z = (int)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24)) - 510;
    return (z * sigma * 443 + 32768) >> 16;
}

template <int PASS>
__global__ __launch_bounds__(kThreads) void augment_pass_kernel(
    const float* __restrict__ rgb, const float* __restrict__ depth, const uint8_t* __restrict__ mask,
    const uint8_t* __restrict__ bg_rgb, const float* __restrict__ bg_depth, const uint8_t* __restrict__ bg_mask,
    const uint8_t* __restrict__ enable, int S, int Nb, int Hb, int Wb, uint32_t seed, const uint32_t* __restrict__ seed_dev, int force,
    uint32_t* __restrict__ ws, float* __restrict__ out_rgb, float* __restrict__ out_depth)
{
    __shared__ uint32_t buf[2][kExt * kPitch];
    __shared__ PassParams pp;

    const int b = blockIdx.y, t = threadIdx.x;
    const int tiles_x = (S + kTile - 1) / kTile;
    const int x0 = (blockIdx.x % tiles_x) * kTile, y0 = (blockIdx.x / tiles_x) * kTile;
    const int tw = min(kTile, S - x0), th = min(kTile, S - y0);            // the tile, clipped to the image
    const long plane = (long)S * S;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.224f};

    if (enable && enable[b] == 0) {                                        // uniform in the block: the crop is copied bit for bit
        if (PASS == 1) {
            for (int i = t; i < tw * th; i += kThreads) {
                const int ly = i / tw, lx = i - ly * tw;
                const long o = (long)(y0 + ly) * S + (x0 + lx);
#pragma unroll
                for (int c = 0; c < 3; ++c) out_rgb[((long)b * 3 + c) * plane + o] = rgb[((long)b * 3 + c) * plane + o];
                out_depth[(long)b * plane + o] = depth[(long)b * plane + o];
            }
        }
        return;
    }

    if (t == 0) {
        const uint32_t hb = mix32(mix32((seed_dev ? *seed_dev : seed) ^ 0x85ebca6bu) ^ (uint32_t)b);
        pp.active = PASS == 0 ? 1 : (force || mix32(hb ^ 32u) > kP20);
        pp.sharpen = pp.motion = pp.gauss_r = pp.reach_m = 0;
        if (pp.active) draw_pass(hb, PASS, force, pp);
        if (PASS == 1 && bg_rgb) {
            pp.bank = (int)(mix32(hb ^ 33u) % (uint32_t)Nb);
            pp.wy = (int)(mix32(hb ^ 34u) % (uint32_t)(Hb - S - 1));
            pp.wx = (int)(mix32(hb ^ 35u) % (uint32_t)(Wb - S - 1));
        }
    }
    __syncthreads();
    const bool active = pp.active != 0;
    const int h_g = pp.gauss_r, h_m = pp.motion ? pp.reach_m : 0, h_s = pp.sharpen ? 1 : 0;
    const int H = h_s + h_m + h_g;                                         // <= kMaxHalo
    const int ox = x0 - H, oy = y0 - H;                                    // image coordinates of LDS position (0, 0)

    // the load: the tile extended by H, clipped to the image; levels (pass 0) or the workspace and the paste (pass 1); then the gain
    {
        const int rx0 = max(0, x0 - H), ry0 = max(0, y0 - H);
        const int rw = min(S, x0 + kTile + H) - rx0, rh = min(S, y0 + kTile + H) - ry0;
        for (int i = t; i < rw * rh; i += kThreads) {
            const int ly = i / rw, y = ry0 + ly, x = rx0 + (i - ly * rw);
            const long o = (long)y * S + x;
            uint32_t v;
            if (PASS == 0) {
                v = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float f = ((rgb[((long)b * 3 + c) * plane + o] * stdv[c]) + mean[c]) * 255.0f;
                    f = fminf(fmaxf(f, 0.f), 255.f);                       // fmaxf(NaN, 0) = 0
                    v |= (uint32_t)(int)rintf(f) << (8 * c);
                }
            } else {
                v = ws[(long)b * plane + o];
                if (bg_rgb && mask[(long)b * plane + o] == 0) {
                    const long q = ((long)pp.bank * Hb + (pp.wy + y)) * Wb + (pp.wx + x);
                    const uint8_t* s = bg_rgb + q * 3;
                    v = bg_mask[q] < 255 ? ((uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16)) : 0u;
                }
            }
            if (active) v = hsv_gain((int)(v & 255u), (int)((v >> 8) & 255u), (int)((v >> 16) & 255u), pp.ks, pp.kv);
            buf[0][(y - oy) * kPitch + (x - ox)] = v;
        }
    }
    __syncthreads();
    int cur = 0;

    // stage k writes the tile extended by `h`, the reach of the stages after it, clipped to the image
    auto stage = [&](int h, auto&& pixel) {
        const int rx0 = max(0, x0 - h), ry0 = max(0, y0 - h);
        const int rw = min(S, x0 + kTile + h) - rx0, rh = min(S, y0 + kTile + h) - ry0;
        const uint32_t* src = buf[cur];
        uint32_t* dst = buf[cur ^ 1];
        for (int i = t; i < rw * rh; i += kThreads) {
            const int ly = i / rw, y = ry0 + ly, x = rx0 + (i - ly * rw);
            dst[(y - oy) * kPitch + (x - ox)] = pixel(src, y, x);
        }
        __syncthreads();
        cur ^= 1;
    };

    if (pp.sharpen) {
        const int c256 = pp.sh_c, q = pp.sh_q;
        stage(h_m + h_g, [&](const uint32_t* src, int y, int x) {
            int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int row = (reflect101(y + dy, S) - oy) * kPitch - ox;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dy == 0 && dx == 0) continue;
                    const uint32_t v = src[row + reflect101(x + dx, S)];
                    s0 += (int)(v & 255u); s1 += (int)((v >> 8) & 255u); s2 += (int)((v >> 16) & 255u);
                }
            }
            const uint32_t c = src[(y - oy) * kPitch + (x - ox)];
            auto one = [&](int v, int s) {
                const int tt = 2 * (c256 * v - 256 * s) + q;
                return (uint32_t)(tt < 0 ? 0 : min(255, tt / (2 * q)));
            };
            return one((int)(c & 255u), s0) | (one((int)((c >> 8) & 255u), s1) << 8) | (one((int)((c >> 16) & 255u), s2) << 16);
        });
    }
    if (pp.motion) {
        const int n = pp.n_taps;
        stage(h_g, [&](const uint32_t* src, int y, int x) {
            int s0 = 0, s1 = 0, s2 = 0;
            for (int k = 0; k < n; ++k) {
                const uint32_t v = src[(reflect101(y + pp.tap_dy[k], S) - oy) * kPitch + (reflect101(x + pp.tap_dx[k], S) - ox)];
                s0 += (int)(v & 255u); s1 += (int)((v >> 8) & 255u); s2 += (int)((v >> 16) & 255u);
            }
            const int hn = n >> 1;
            return (uint32_t)((s0 + hn) / n) | ((uint32_t)((s1 + hn) / n) << 8) | ((uint32_t)((s2 + hn) / n) << 16);
        });
    }
    if (pp.gauss_r) {
        const int r = pp.gauss_r, w0 = pp.gw[0], w1 = pp.gw[1], w2 = pp.gw[2];
        stage(0, [&](const uint32_t* src, int y, int x) {
            int s0 = 0, s1 = 0, s2 = 0;
            for (int dy = -r; dy <= r; ++dy) {
                const int ady = dy < 0 ? -dy : dy, wy = ady == 0 ? w0 : (ady == 1 ? w1 : w2);
                const int row = (reflect101(y + dy, S) - oy) * kPitch - ox;
                for (int dx = -r; dx <= r; ++dx) {
                    const int adx = dx < 0 ? -dx : dx, w = wy * (adx == 0 ? w0 : (adx == 1 ? w1 : w2));
                    const uint32_t v = src[row + reflect101(x + dx, S)];
                    s0 += w * (int)(v & 255u); s1 += w * (int)((v >> 8) & 255u); s2 += w * (int)((v >> 16) & 255u);
                }
            }
            return (uint32_t)((s0 + 32768) >> 16) | ((uint32_t)((s1 + 32768) >> 16) << 8) | ((uint32_t)((s2 + 32768) >> 16) << 16);
        });
    }

    // the store: noise, then the workspace (pass 0) or the normalised crop and the pasted depth (pass 1)
    const uint32_t* fin = buf[cur];
    for (int i = t; i < tw * th; i += kThreads) {
        const int ly = i / tw, y = y0 + ly, x = x0 + (i - ly * tw);
        const long o = (long)y * S + x;
        const uint32_t v = fin[(y - oy) * kPitch + (x - ox)];
        int ch[3] = {(int)(v & 255u), (int)((v >> 8) & 255u), (int)((v >> 16) & 255u)};
        if (active) {
            const uint32_t p3 = 3u * (uint32_t)o;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int u = ch[c] + noise_of(mix32(pp.hs0 ^ (p3 + (uint32_t)c)), pp.sigma);
                u = min(255, max(0, u));
                if (pp.extra) u = min(255, max(0, u + noise_of(mix32(pp.hs1 ^ (p3 + (uint32_t)c)), 7)));
                ch[c] = u;
            }
        }
        if (PASS == 0) {
            ws[(long)b * plane + o] = (uint32_t)ch[0] | ((uint32_t)ch[1] << 8) | ((uint32_t)ch[2] << 16);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float f = (float)ch[c] / 255.0f;
                f = f - mean[c];
                out_rgb[((long)b * 3 + c) * plane + o] = f / stdv[c];
            }
            float d = depth[(long)b * plane + o];
            if (bg_rgb && !(d > 1e-6f)) {
                const long q = ((long)pp.bank * Hb + (pp.wy + y)) * Wb + (pp.wx + x);
                d = bg_mask[q] < 255 ? bg_depth[q] : 0.0f;
            }
            out_depth[(long)b * plane + o] = d;
        }
    }
}

__global__ void dzi_boxes_kernel(const float* __restrict__ bbox, int B, float max_side, float pad_ratio, float scale_ratio,
                                 float shift_ratio, int train, uint32_t seed, const uint32_t* __restrict__ seed_dev,
                                 float* __restrict__ center, float* __restrict__ scale)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float x1 = bbox[4 * b], y1 = bbox[4 * b + 1], x2 = bbox[4 * b + 2], y2 = bbox[4 * b + 3];
    const float bw = x2 - x1, bh = y2 - y1;
    float cx = 0.5f * (x1 + x2), cy = 0.5f * (y1 + y2);
    const float m = (bh > bw || bh != bh) ? bh : bw;
    float s;
    if (train) {
        const uint32_t hb = mix32(mix32((seed_dev ? *seed_dev : seed) ^ 0xc2b2ae35u) ^ (uint32_t)b);
        float u[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) u[k] = 2.0f * ((float)(mix32(hb ^ (uint32_t)k) >> 8) * 5.9604644775390625e-8f) - 1.0f;
        cx = cx + bw * (shift_ratio * u[1]);
        cy = cy + bh * (shift_ratio * u[2]);
        s = (m * (1.0f + scale_ratio * u[0])) * pad_ratio;
    } else {
        s = m * pad_ratio;
    }
    center[2 * b] = cx;
    center[2 * b + 1] = cy;
    scale[b] = s > max_side ? max_side : s;
}

} // namespace

static int g_force_all = 0;

extern "C" void gdm_augment_force_all_stages(int on) { g_force_all = on != 0; }

extern "C" size_t gdm_augment_workspace_bytes(int B, int S)
{
    if (B < 1 || B > 65535 || S < GDM_AUG_MIN_S || S > GDM_AUG_MAX_S) return 0;
    return (size_t)B * (size_t)S * (size_t)S * 4;
}

extern "C" int gdm_augment_crops_hip(const float* rgb, const float* depth, const uint8_t* mask, const uint8_t* bg_rgb,
                                     const float* bg_depth, const uint8_t* bg_mask, const uint8_t* enable, int B, int S, int Nb, int Hb,
                                     int Wb, uint32_t seed, const uint32_t* seed_dev, float* out_rgb, float* out_depth, void* workspace,
                                     size_t workspace_bytes, void* stream)
{
    GDM_CHECK_ARG(rgb && depth && out_rgb && out_depth && workspace, "gdm_augment_crops_hip: NULL pointer");
    GDM_CHECK_ARG((bg_rgb == nullptr) == (bg_depth == nullptr) && (bg_rgb == nullptr) == (bg_mask == nullptr),
                  "gdm_augment_crops_hip: bg_rgb, bg_depth and bg_mask go together (all or none)");
    GDM_CHECK_ARG(!bg_rgb || mask, "gdm_augment_crops_hip: the paste needs the crop's mask (NULL)");
    GDM_CHECK_ARG(out_rgb != rgb && out_depth != depth, "gdm_augment_crops_hip: an output aliases its input");
    GDM_CHECK_ARG(B >= 1 && B <= 65535, "gdm_augment_crops_hip: B=%d not in [1, 65535]", B);
    GDM_CHECK_ARG(S >= GDM_AUG_MIN_S && S <= GDM_AUG_MAX_S, "gdm_augment_crops_hip: S=%d not in [%d, %d]", S, GDM_AUG_MIN_S,
                  GDM_AUG_MAX_S);
    if (bg_rgb) {
        GDM_CHECK_ARG(Nb >= 1, "gdm_augment_crops_hip: Nb=%d must be at least 1", Nb);
        GDM_CHECK_ARG(Hb >= S + 2 && Wb >= S + 2 && Hb <= 65536 && Wb <= 65536,
                      "gdm_augment_crops_hip: the bank's frames are %d x %d, S + 2 = %d (and at most 65536) a side needed", Hb, Wb, S + 2);
    }
    const size_t need = gdm_augment_workspace_bytes(B, S);
    GDM_CHECK_ARG(workspace_bytes >= need, "gdm_augment_crops_hip: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    GDM_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "gdm_augment_crops_hip: workspace must be 4-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const int tiles = (S + kTile - 1) / kTile;
    const dim3 grid(tiles * tiles, B);
    hipLaunchKernelGGL(augment_pass_kernel<0>, grid, dim3(kThreads), 0, s, rgb, depth, mask, bg_rgb, bg_depth, bg_mask, enable, S, Nb, Hb,
                       Wb, seed, seed_dev, g_force_all, (uint32_t*)workspace, out_rgb, out_depth);
    int rc = gdm_launch_status("augment_pass_kernel<0>");
    if (rc) return rc;
    hipLaunchKernelGGL(augment_pass_kernel<1>, grid, dim3(kThreads), 0, s, rgb, depth, mask, bg_rgb, bg_depth, bg_mask, enable, S, Nb, Hb,
                       Wb, seed, seed_dev, g_force_all, (uint32_t*)workspace, out_rgb, out_depth);
    return gdm_launch_status("augment_pass_kernel<1>");
}

extern "C" int gdm_dzi_boxes_hip(const float* bbox, int B, float max_side, float pad_ratio, float scale_ratio, float shift_ratio,
                                 int train, uint32_t seed, const uint32_t* seed_dev, float* center, float* scale, void* stream)
{
    GDM_CHECK_ARG(bbox && center && scale, "gdm_dzi_boxes_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1, "gdm_dzi_boxes_hip: B=%d must be at least 1", B);
    hipLaunchKernelGGL(dzi_boxes_kernel, dim3(gdm_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, bbox, B, max_side, pad_ratio,
                       scale_ratio, shift_ratio, train, seed, seed_dev, center, scale);
    return gdm_launch_status("dzi_boxes_kernel");
}
