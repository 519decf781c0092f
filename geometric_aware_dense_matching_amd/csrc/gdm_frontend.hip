// Front end on the device, gfx950: from the raw frame and a detection box to the crop the model takes, the two steps the reference
// loader does on the host for every item (datasets/lm/linemod_pbr.py:460-473).
//   depth_normals_kernel   the surface normal of every pixel from the uint16 millimetre depth: the LINEMOD least-squares depth gradient
//                          over the 8 taps at distance k_size, in integers up to the final fp32 scaling and normalisation
//   warp_crop_kernel       the S x S crop around (center, scale): OpenCV's fixed-point warpAffine for a pure scale + shift, bilinear for
//                          rgb (uint8, then normalize_color) and normals, nearest for depth, mask and the dpt_2_pcld point of the pixel;
//                          the source coordinate is formed once per output pixel and shared by all five outputs
// Both are one launch for the batch, one pixel per thread, x fastest.  Every load is bounds-checked against the frame.  No allocation
// and no host synchronisation: both capture in a hipGraph.
// The arithmetic is stated operation by operation in include/gdm.h; this file is compiled without fp contraction.
#include "gdm_common.h"

namespace {

// (uint16) trunc(depth * 1000): negative and NaN -> 0, 65.535 m and beyond -> 65535 (include/gdm.h).
__device__ __forceinline__ int depth_mm(float d)
{
    const float v = d * 1000.0f;
    return v >= 65535.0f ? 65535 : (v >= 0.0f ? (int)v : 0);
}

// One pixel per thread: a wave's nine tap loads and three stores are each 256 contiguous bytes (four pixels per thread with float4
// stores stride the tap loads by 16 bytes and measured 1.5 times slower).
// Every tap offset is 0 or +-r, so A = r^2 A' and b = r b' with A', b' summed over the signs (ii, jj).  A', b' and their products
// fit 32 bits (|b'| <= 6 * 65535); det = r^4 det' and dd = r^3 dd' are formed in fp64, exactly (< 2^53), and rounded to fp32 once:
// the values of the 64-bit integer expressions of include/gdm.h, without their 64-bit multiplies and conversions (measured 32 us
// against 41 us per 16 frames).
__global__ __launch_bounds__(256) void depth_normals_kernel(const float* __restrict__ depth, const float* __restrict__ K, int H, int W,
                                                            int r, int dist_thr, int diff_thr, float* __restrict__ out)
{
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= H * W) return;
    const int y = t / W, x = t % W;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (x >= r && x < W - r && y >= r && y < H - r) {                      // so every tap below lies inside the frame
        const float* ctr = depth + ((long)b * H + y) * W + x;
        const int rW = r * W;
        const int c = depth_mm(ctr[0]);
        if (c < dist_thr) {
            int A0 = 0, A1 = 0, A3 = 0, b0 = 0, b1 = 0;
#pragma unroll
            for (int jj = -1; jj <= 1; ++jj) {
#pragma unroll
                for (int ii = -1; ii <= 1; ++ii) {
                    if (ii == 0 && jj == 0) continue;
                    const int delta = depth_mm(ctr[jj * rW + ii * r]) - c;
                    if (abs(delta) < diff_thr) {
                        A0 += ii * ii; A1 += ii * jj; A3 += jj * jj;
                        b0 += ii * delta; b1 += jj * delta;
                    }
                }
            }
            const int det = A0 * A3 - A1 * A1, ddx = A3 * b0 - A1 * b1, ddy = -A1 * b0 + A0 * b1;
            const double r3 = ((double)r * (double)r) * (double)r, r4 = r3 * (double)r;
            const float gx = K[b * 9] * (float)(r3 * (double)ddx), gy = K[b * 9 + 4] * (float)(r3 * (double)ddy);
            const float gz = (float)(-(r4 * (double)(det * c)));
            const float s = sqrtf((gx * gx + gy * gy) + gz * gz);
            if (s > 0.f) { nx = gx / s; ny = gy / s; nz = gz / s; }
        }
    }
    const long plane = (long)H * W;
    float* o = out + (long)b * 3 * plane + t;
    o[0] = nx; o[plane] = ny; o[2 * plane] = nz;
}

// round-half-even(v * 1024) as an integer; NaN and anything beyond +-1e15 land on +-1e15 (far outside any frame).
__device__ __forceinline__ long long fix10(double v)
{
    return llrint(fmin(fmax(v * 1024.0, -1e15), 1e15));
}

// One output pixel per thread, x fastest: a wave's tap loads follow the source row and its stores to the planar outputs are 256
// contiguous bytes.  (Four pixels per thread with float4 / uchar4 stores measured slower, 22-26 us against 17 us per 16 crops: the
// tap loads of a wave then spread over four times as many cache lines.)
__global__ __launch_bounds__(256) void warp_crop_kernel(const uint8_t* __restrict__ rgb, const float* __restrict__ depth,
                                                        const float* __restrict__ normals, const float* __restrict__ K,
                                                        const uint8_t* __restrict__ mask, const float* __restrict__ center,
                                                        const float* __restrict__ scale, int H, int W, int S, float* __restrict__ o_rgb,
                                                        float* __restrict__ o_nrm, float* __restrict__ o_xyz, float* __restrict__ o_dep,
                                                        uint8_t* __restrict__ o_msk)
{
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= S * S) return;
    const int y = t / S, x = t % S;
    // dst (x, y) -> src (a x + bx, a y + by): get_affine_transform with rot = 0, inverted in closed form, fp64
    const double a = (double)scale[b] / (double)S;
    const double half = (a * (double)S) / 2.0;
    const double bx = (double)center[2 * b] - half, by = (double)center[2 * b + 1] - half;
    const long long rx = fix10(a * (double)x) + fix10(bx), ry = fix10(a * (double)y + by);
    const long long X = (rx + 512) >> 10, Y = (ry + 512) >> 10;           // nearest
    const long long X5 = (rx + 16) >> 5, Y5 = (ry + 16) >> 5;             // linear: 5 fraction bits
    const long long sx = X5 >> 5, sy = Y5 >> 5;
    const int al = (int)(X5 & 31), be = (int)(Y5 & 31);
    const bool row0 = sy >= 0 && sy < H, row1 = sy + 1 >= 0 && sy + 1 < H;
    const bool col0 = sx >= 0 && sx < W, col1 = sx + 1 >= 0 && sx + 1 < W;
    const bool in[4] = {row0 && col0, row0 && col1, row1 && col0, row1 && col1};
    long off[4];                                                           // formed only for taps inside the frame
    off[0] = in[0] ? sy * W + sx : 0;
    off[1] = in[1] ? sy * W + sx + 1 : 0;
    off[2] = in[2] ? (sy + 1) * W + sx : 0;
    off[3] = in[3] ? (sy + 1) * W + sx + 1 : 0;
    const long plane = (long)H * W, oplane = (long)S * S;
    const long pix = (long)b * oplane + t;                                 // this pixel in a [B,S,S] output

    // rgb: uint8 taps blended in fixed point (the 1/32-step weight products scaled to 2^15), then normalize_color with the crop std
    const uint8_t* rgb_b = rgb + (long)b * plane * 3;
    const int wi[4] = {32 * (32 - be) * (32 - al), 32 * (32 - be) * al, 32 * be * (32 - al), 32 * be * al};
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (in[q]) {
            const uint8_t* s = rgb_b + off[q] * 3;
            acc[0] += wi[q] * (int)s[0]; acc[1] += wi[q] * (int)s[1]; acc[2] += wi[q] * (int)s[2];
        }
    }
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.224f};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float f = (float)((acc[ch] + 16384) >> 15) / 255.0f;
        f = f - mean[ch];
        o_rgb[((long)b * 3 + ch) * oplane + t] = f / stdv[ch];
    }

    // normals: ((v0 w0 + v1 w1) + v2 w2) + v3 w3 in fp32, a tap outside the frame is 0
    if (o_nrm) {                                                           // uniform: the YCB-V item takes its normals from the crop
        const float* nrm_b = normals + (long)b * 3 * plane;
        const float fb = (float)be / 32.0f, fa = (float)al / 32.0f;
        const float wf[4] = {(1.0f - fb) * (1.0f - fa), (1.0f - fb) * fa, fb * (1.0f - fa), fb * fa};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = nrm_b + ch * plane;
            const float v0 = in[0] ? s[off[0]] : 0.f, v1 = in[1] ? s[off[1]] : 0.f;
            const float v2 = in[2] ? s[off[2]] : 0.f, v3 = in[3] ? s[off[3]] : 0.f;
            o_nrm[((long)b * 3 + ch) * oplane + t] = ((v0 * wf[0] + v1 * wf[1]) + v2 * wf[2]) + v3 * wf[3];
        }
    }

    // nearest: depth, mask, and dpt_2_pcld of the source pixel (the arithmetic of depth_to_xyz_kernel)
    const bool inn = Y >= 0 && Y < H && X >= 0 && X < W;
    const long offn = inn ? Y * W + X : 0;
    const float d = inn ? depth[(long)b * plane + offn] : 0.f;
    o_dep[pix] = d;
    if (o_msk) o_msk[pix] = inn ? mask[(long)b * plane + offn] : (uint8_t)0;
    const float* k = K + b * 9;
    const float kfx = k[0], kcx = k[2], kfy = k[4], kcy = k[5];
    const double m = d > 1e-8f ? 1.0 : 0.0;
    float* ox = o_xyz + pix * 3;
    ox[0] = (float)(((double)X - (double)kcx) * (double)d / (double)kfx * m);
    ox[1] = (float)(((double)Y - (double)kcy) * (double)d / (double)kfy * m);
    ox[2] = (float)((double)d * m);
}

} // namespace

extern "C" int gdm_depth_normals_hip(const float* depth, const float* K, int B, int H, int W, int k_size, int distance_threshold,
                                     int difference_threshold, float* normals, void* stream)
{
    GDM_CHECK_ARG(depth && K && normals, "gdm_depth_normals_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768,
                  "gdm_depth_normals_hip: bad shape B=%d H=%d W=%d", B, H, W);
    GDM_CHECK_ARG(k_size >= 1 && k_size <= GDM_NORMALS_MAX_K, "gdm_depth_normals_hip: k_size=%d not in [1, %d]", k_size,
                  GDM_NORMALS_MAX_K);
    GDM_CHECK_ARG(distance_threshold >= 0 && distance_threshold <= 65536 && difference_threshold >= 0 && difference_threshold <= 65536,
                  "gdm_depth_normals_hip: thresholds %d, %d not in [0, 65536]", distance_threshold, difference_threshold);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_normals_kernel, dim3(gdm_cdiv((long)H * W, 256), B), dim3(256), 0, s, depth, K, H, W, k_size,
                       distance_threshold, difference_threshold, normals);
    return gdm_launch_status("depth_normals_kernel");
}

extern "C" int gdm_warp_crop_hip(const uint8_t* rgb, const float* depth, const float* normals, const float* K, const uint8_t* mask,
                                 const float* center, const float* scale, int B, int H, int W, int S, float* out_rgb,
                                 float* out_normals, float* out_xyz, float* out_depth, uint8_t* out_mask, void* stream)
{
    GDM_CHECK_ARG(rgb && depth && K && center && scale && out_rgb && out_xyz && out_depth, "gdm_warp_crop_hip: NULL pointer");
    GDM_CHECK_ARG((normals == nullptr) == (out_normals == nullptr),
                  "gdm_warp_crop_hip: normals and out_normals go together (both or neither)");
    GDM_CHECK_ARG((mask == nullptr) == (out_mask == nullptr), "gdm_warp_crop_hip: mask and out_mask go together (both or neither)");
    GDM_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "gdm_warp_crop_hip: bad shape B=%d H=%d W=%d",
                  B, H, W);
    GDM_CHECK_ARG(S >= 1 && S <= 16384, "gdm_warp_crop_hip: S=%d not in [1, 16384]", S);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(warp_crop_kernel, dim3(gdm_cdiv((long)S * S, 256), B), dim3(256), 0, s, rgb, depth, normals, K, mask, center, scale,
                       H, W, S, out_rgb, out_normals, out_xyz, out_depth, out_mask);
    return gdm_launch_status("warp_crop_kernel");
}
