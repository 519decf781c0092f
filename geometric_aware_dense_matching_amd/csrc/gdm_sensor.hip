// A structured-light depth sensor on a metric depth frame, gfx950: THE SENSOR RULE of include/gdm.h (gdm_depth_sensor_hip), one launch
// for the batch, one workgroup of four waves per (frame, 128 x 8 tile).
//   z1   the depth that survives stage 1 (0 empty, -1 out of range), the tile with a ring of 2 and Wd further columns on the projector
//        side: stage 4 reads stage-3 results one pixel away, stage 3 reads stage-1 depth one pixel further, and a pixel of the ring of 1
//        needs the g of the Wd pixels beside it
//   gm   g of the ring-of-1 rows (its negative for a negative baseline, so that both signs take a minimum; +inf where nothing survives),
//        turned in place into the minima over 2^k neighbours by log-step doubling: every thread reads its (at most kPer) pairs into
//        registers, the workgroup synchronises, then it writes.  The window of Wd is two overlapping spans of 2^K, K = floor(log2 Wd)
//   z3   the ring of 1 after stages 1 - 3: the depth, or minus the cause
// The halo is recomputed, never exchanged.  LDS: 12 x 387 + 10 x 387 + 10 x 130 floats = 39256 bytes, four workgroups to a CU; lanes
// walk a row, i.e. consecutive banks, in every pass.  The intrinsics of at most GDM_SENSOR_MAX_K frames travel by value.
#include "gdm_common.h"
#include <math.h>

namespace {

constexpr int kTW = GDM_SENSOR_TILE_W, kTH = GDM_SENSOR_TILE_H, kThreads = 256;
constexpr int kCols = kTW + 4 + GDM_SENSOR_MAX_DISP;                       // 387
constexpr int kRowsZ = kTH + 4, kRowsG = kTH + 2, kCols3 = kTW + 2;        // 12, 10, 130
constexpr int kPer = (kRowsG * kCols + kThreads - 1) / kThreads;           // 16 pairs a thread at Wd = 255
constexpr float kUnit = 0.0067658751f;                                     // 1 / sqrt(21845)

struct FrameK {
    float fx, fy, cx, cy, fb;
    int wd;
};
struct SensorK {
    FrameK k[GDM_SENSOR_MAX_K];
};

__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// g of the rule for a positive baseline, its negative for a negative one: "x' shadows x" is gval(x') <= gval(x) for both
__device__ __forceinline__ float gval(int x, float z, float fb, int neg)
{
    const float D = fb / z;
    return neg ? -((float)x + D) : (float)x - D;
}

struct P3 {
    float x, y, z;
};
__device__ __forceinline__ P3 backproject(int x, int y, float z, const FrameK& k)
{
    const float u = ((float)x - k.cx) / k.fx, v = ((float)y - k.cy) / k.fy;
    return {z * u, z * v, z};
}
__device__ __forceinline__ P3 sub(const P3& a, const P3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(const P3& a, const P3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

__global__ __launch_bounds__(kThreads) void depth_sensor_kernel(
    const float* __restrict__ depth, const SensorK ka, int k_per_frame, int H, int W, int neg, float z_min, float z_max, float sigma_d,
    float subpixel, float cmin2, float csoft2, uint32_t t_shift, int stages, uint32_t seed, const uint32_t* __restrict__ seed_dev,
    float* __restrict__ out_depth, uint8_t* __restrict__ cause)
{
    __shared__ float z1[kRowsZ * kCols];
    __shared__ float gm[kRowsG * kCols];
    __shared__ float z3[kRowsG * kCols3];

    const int b = blockIdx.y, t = threadIdx.x;
    const int tiles_x = (W + kTW - 1) / kTW;
    const int x0 = (blockIdx.x % tiles_x) * kTW, y0 = (blockIdx.x / tiles_x) * kTH;
    const FrameK fk = ka.k[k_per_frame ? b : 0];
    const bool shadow = (stages & GDM_SENSOR_SHADOW) != 0;
    const int wd = shadow ? min(max(fk.wd, 1), GDM_SENSOR_MAX_DISP) : 0;   // the entry refused anything else
    const int cw = kTW + 4 + wd;                                           // <= kCols
    const uint32_t cw_inv = 0xffffffffu / (uint32_t)cw + 1u;               // ceil(2^32 / cw): __umulhi(i, cw_inv) = i / cw for i < 2^32 / cw
    const int ox = x0 - 2 - (neg ? wd : 0), oy = y0 - 2;                   // image coordinates of z1's (0, 0)
    const int dir = neg ? -1 : 1;                                          // where the pixels that can shadow this one lie
    const long plane = (long)H * W;
    const float* dz = depth + (long)b * plane;

    // stage 1 into LDS: the tile, the ring of 2 and the window
    for (int i = t; i < kRowsZ * cw; i += kThreads) {
        const int r = (int)__umulhi((uint32_t)i, cw_inv), lc = i - r * cw, y = oy + r, x = ox + lc;
        float v = 0.f;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const float z = dz[(long)y * W + x];
            if (z > 0.f) v = ((stages & GDM_SENSOR_RANGE) && !(z >= z_min && z <= z_max)) ? -1.f : z;
        }
        z1[r * kCols + lc] = v;
    }
    __syncthreads();

    // stage 2: gm <- g, then the minima over 2^K pixels from each position towards the projector side
    int K2 = 0;
    if (shadow) {
        for (int i = t; i < kRowsG * cw; i += kThreads) {
            const int r = (int)__umulhi((uint32_t)i, cw_inv), lc = i - r * cw;
            const float z = z1[(r + 1) * kCols + lc];
            gm[r * kCols + lc] = z > 0.f ? gval(ox + lc, z, fk.fb, neg) : INFINITY;
        }
        __syncthreads();
        while ((2 << K2) <= wd) ++K2;                                      // floor(log2 wd)
        for (int k = 0, step = 1; k < K2; ++k, step <<= 1) {
            float v[kPer];
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int i = t + j * kThreads;
                v[j] = INFINITY;
                if (i < kRowsG * cw) {
                    const int r = (int)__umulhi((uint32_t)i, cw_inv), lc = i - r * cw, l2 = lc + dir * step;
                    const float a = gm[r * kCols + lc];
                    v[j] = (l2 >= 0 && l2 < cw) ? fminf(a, gm[r * kCols + l2]) : a;
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int i = t + j * kThreads;
                if (i < kRowsG * cw) {
                    const int r = (int)__umulhi((uint32_t)i, cw_inv), lc = i - r * cw;
                    gm[r * kCols + lc] = v[j];
                }
            }
            __syncthreads();
        }
    }

    const uint32_t hb = mix32(mix32((seed_dev ? *seed_dev : seed) ^ 0x27d4eb2fu) ^ (uint32_t)b);
    const uint32_t hs1 = mix32(hb ^ 1u), hs2 = mix32(hb ^ 2u), hs3 = mix32(hb ^ 3u);

    // stages 2 and 3 on the ring of 1: the depth, or minus the cause
    const int lx0 = (x0 - 1) - ox;                                         // 1, or 1 + wd: a column on either side stays inside z1
    for (int i = t; i < kRowsG * kCols3; i += kThreads) {
        const int r3 = i / kCols3, c3 = i - r3 * kCols3, lc = lx0 + c3, rz = r3 + 1, x = x0 - 1 + c3, y = y0 - 1 + r3;
        const float z = z1[rz * kCols + lc];
        float s;
        if (!(z > 0.f)) {
            s = z < 0.f ? -2.f : -1.f;
        } else {
            s = z;
            if (shadow) {                                                  // lc + dir wd lies inside [0, cw) for every ring pixel
                const float m = fminf(gm[r3 * kCols + lc + dir], gm[r3 * kCols + lc + dir * (wd - (1 << K2) + 1)]);
                if (m <= gval(x, z, fk.fb, neg)) s = -3.f;
            }
            if (s > 0.f && (stages & GDM_SENSOR_GRAZING)) {
                const float zl = z1[rz * kCols + lc - 1], zr = z1[rz * kCols + lc + 1];
                const float zu = z1[(rz - 1) * kCols + lc], zd = z1[(rz + 1) * kCols + lc];
                const P3 P = backproject(x, y, z, fk);
                bool have = true;
                P3 tx = P, ty = P;
                if (zl > 0.f && zr > 0.f) tx = sub(backproject(x + 1, y, zr, fk), backproject(x - 1, y, zl, fk));
                else if (zr > 0.f) tx = sub(backproject(x + 1, y, zr, fk), P);
                else if (zl > 0.f) tx = sub(P, backproject(x - 1, y, zl, fk));
                else have = false;
                if (zu > 0.f && zd > 0.f) ty = sub(backproject(x, y + 1, zd, fk), backproject(x, y - 1, zu, fk));
                else if (zd > 0.f) ty = sub(backproject(x, y + 1, zd, fk), P);
                else if (zu > 0.f) ty = sub(P, backproject(x, y - 1, zu, fk));
                else have = false;
                if (!have) {
                    s = -4.f;
                } else {
                    const P3 nrm = {tx.y * ty.z - tx.z * ty.y, tx.z * ty.x - tx.x * ty.z, tx.x * ty.y - tx.y * ty.x};
                    const float np = dot(nrm, P);
                    const float c2 = (np * np) / (dot(nrm, nrm) * dot(P, P));
                    if (!(c2 >= cmin2)) {
                        s = -4.f;
                    } else if (c2 < csoft2) {
                        const float r = (csoft2 - c2) / (csoft2 - cmin2);
                        const uint32_t T = (uint32_t)(r * 16777216.0f);
                        if ((mix32(hs1 ^ (uint32_t)(y * W + x)) >> 8) < T) s = -4.f;
                    }
                }
            }
        }
        z3[i] = s;
    }
    __syncthreads();

    // stages 4 and 5, and the store
    for (int i = t; i < kTW * kTH; i += kThreads) {
        const int ly = i / kTW, lx = i - ly * kTW, x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const uint32_t p = (uint32_t)(y * W + x);
        int jx = 0, jy = 0;
        if (stages & GDM_SENSOR_JITTER) {
            const uint32_t w = mix32(hs2 ^ p), h0 = w & 0xffffu, h1 = w >> 16;
            jx = h0 < t_shift ? -1 : (h0 >= 65536u - t_shift ? 1 : 0);
            jy = h1 < t_shift ? -1 : (h1 >= 65536u - t_shift ? 1 : 0);
        }
        const int qx = x + jx, qy = y + jy;
        float o = 0.f;
        int c = 0;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) {
            c = 5;
        } else {
            const float s = z3[(ly + 1 + jy) * kCols3 + (lx + 1 + jx)];
            if (!(s > 0.f)) {
                c = (int)(-s);
            } else if (stages & GDM_SENSOR_NOISE) {
                const float D = fk.fb / s;
                const uint32_t w = mix32(hs3 ^ p);
                const int zeta = (int)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24)) - 510;
                const float e = (float)zeta * kUnit;
                const float Dn = D + sigma_d * e;
                const float Dq = rintf(Dn * subpixel) / subpixel;
                if (!(Dq > 0.f)) c = 2;
                else o = fk.fb / Dq;
            } else {
                o = s;
            }
        }
        const long at = (long)b * plane + (long)y * W + x;
        out_depth[at] = o;
        cause[at] = (uint8_t)c;
    }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t A = (uintptr_t)a, B = (uintptr_t)b;
    return A < B + nb && B < A + na;
}

} // namespace

extern "C" int gdm_depth_sensor_hip(const float* depth, const float* K, int k_per_frame, int n, int H, int W, float baseline, float z_min,
                                    float z_max, float sigma_d, float subpixel, float cos_min, float cos_soft, float p_shift, int stages,
                                    uint32_t seed, const uint32_t* seed_dev, float* out_depth, uint8_t* cause, void* stream)
{
    GDM_CHECK_ARG(depth && K && out_depth && cause, "gdm_depth_sensor_hip: NULL pointer");
    GDM_CHECK_ARG(n >= 1 && n <= 65535, "gdm_depth_sensor_hip: n=%d not in [1, 65535]", n);
    GDM_CHECK_ARG(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "gdm_depth_sensor_hip: H=%d, W=%d not in [1, 16384]", H, W);
    GDM_CHECK_ARG(k_per_frame == 0 || k_per_frame == 1, "gdm_depth_sensor_hip: k_per_frame=%d must be 0 or 1", k_per_frame);
    GDM_CHECK_ARG(!k_per_frame || n <= GDM_SENSOR_MAX_K, "gdm_depth_sensor_hip: n=%d frames with a K each, at most %d travel", n,
                  GDM_SENSOR_MAX_K);
    GDM_CHECK_ARG(stages >= 0 && stages <= 31, "gdm_depth_sensor_hip: stages=%d not in [0, 31]", stages);
    GDM_CHECK_ARG(isfinite(baseline) && baseline != 0.f, "gdm_depth_sensor_hip: baseline=%g must be finite and not 0", baseline);
    GDM_CHECK_ARG(z_min > 0.f && isfinite(z_min), "gdm_depth_sensor_hip: z_min=%g must be positive", z_min);
    GDM_CHECK_ARG(z_max > z_min, "gdm_depth_sensor_hip: z_max=%g must exceed z_min=%g", z_max, z_min);
    GDM_CHECK_ARG(sigma_d >= 0.f && isfinite(sigma_d), "gdm_depth_sensor_hip: sigma_d=%g must be finite and not negative", sigma_d);
    GDM_CHECK_ARG(subpixel >= 1.f && isfinite(subpixel), "gdm_depth_sensor_hip: subpixel=%g must be at least 1", subpixel);
    GDM_CHECK_ARG(cos_min >= 0.f && cos_soft <= 1.f && cos_soft >= cos_min,
                  "gdm_depth_sensor_hip: 0 <= cos_min=%g <= cos_soft=%g <= 1 needed", cos_min, cos_soft);
    GDM_CHECK_ARG(p_shift >= 0.f && p_shift <= 1.f, "gdm_depth_sensor_hip: p_shift=%g is no probability", p_shift);
    SensorK ka = {};
    for (int i = 0; i < (k_per_frame ? n : 1); ++i) {
        FrameK& k = ka.k[i];
        k.fx = K[9 * i], k.cx = K[9 * i + 2], k.fy = K[9 * i + 4], k.cy = K[9 * i + 5];
        GDM_CHECK_ARG(k.fx > 0.f && k.fy > 0.f && isfinite(k.fx) && isfinite(k.fy) && isfinite(k.cx) && isfinite(k.cy),
                      "gdm_depth_sensor_hip: K of frame %d: fx=%g, fy=%g must be positive and finite, cx, cy finite", i, k.fx, k.fy);
        k.fb = (float)((double)k.fx * (double)fabsf(baseline));
        const float w = ceilf(k.fb / z_min);
        GDM_CHECK_ARG(w >= 1.f && w <= (float)GDM_SENSOR_MAX_DISP,
                      "gdm_depth_sensor_hip: frame %d: the shadow window ceil(fx |baseline| / z_min) = %g not in [1, %d]", i, w,
                      GDM_SENSOR_MAX_DISP);
        k.wd = (int)w;
    }
    const size_t px = (size_t)n * H * W;
    GDM_CHECK_ARG(!overlap(depth, px * 4, out_depth, px * 4) && !overlap(depth, px * 4, cause, px) && !overlap(out_depth, px * 4, cause, px),
                  "gdm_depth_sensor_hip: out_depth and cause may overlap neither depth nor each other (aliased)");
    const dim3 grid(gdm_cdiv(W, kTW) * gdm_cdiv(H, kTH), n);
    hipLaunchKernelGGL(depth_sensor_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, depth, ka, k_per_frame, H, W,
                       baseline < 0.f ? 1 : 0, z_min, z_max, sigma_d, subpixel, cos_min * cos_min, cos_soft * cos_soft,
                       (uint32_t)(p_shift * 32768.0f), stages, seed, seed_dev, out_depth, cause);
    return gdm_launch_status("depth_sensor_kernel");
}
