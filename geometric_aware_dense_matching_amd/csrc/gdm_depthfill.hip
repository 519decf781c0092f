// Depth completion on the device, gfx950: the hole filling the YCB-V loader applies to every cropped depth image on the host
// (datasets/ycbv/ycbv_pbr.py:477, IP-Basic's fill_in_multiscale / fill_in_fast).  The operator is a chain of small stencils (dilate,
// erode, 5 x 5 median, bilateral) with two column scans in the multiscale form; the planes are small and stay in L2, so the launch count
// and the dependency depth cost the time.  Each kernel therefore keeps a tile with its ring in LDS, two buffers, and runs its stencils
// back to back, each over a ring narrower by its own radius:
//   fill_ms_head_kernel   s1 .. s4 (invert, three binned cross dilations, 5 x 5 close, median), ring 9; column tops of s4 by atomicMin
//   fill_ms_hole_kernel   s5 (the 9 x 9 fill under the top mask), straight from L2; column tops of s5 by atomicMin
//   fill_ms_tail_kernel   six masked 5 x 5 dilations, median, bilateral, inversion, ring 16
//   fill_fast_kernel      the whole fast form, ring 13
// The launches split where a column scan has to be complete.  A stage applies ITS OWN border rule at the IMAGE edge (ignore /
// replicate / reflect-101): every tap is mapped into the image first, a ring position outside the image is never computed and never
// read.  A column without a valid pixel has top row 0 (the reference's np.argmax of all-False): the tables start at a sentinel that
// the readers map to 0.
// The arithmetic is stated operation by operation in include/gdm.h; this file is compiled without fp contraction.  No allocation and
// no host synchronisation: the calls capture in a hipGraph (one memset node and three kernels, or one kernel).
#include "gdm_common.h"
#include <math.h>

namespace {

constexpr int NT = 256;                    // threads per workgroup
constexpr int TOP_NONE = 0x7f7f7f7f;       // what hipMemsetAsync(0x7f) leaves: no valid pixel seen in the column

struct Bilateral { float cc, w0, w1, w2, w4; };          // -1 / (2 sigma_c^2) and the spatial weights at dx^2 + dy^2 = 0, 1, 2, 4

__device__ __forceinline__ float clean(float d) { return d > 0.0f ? d : 0.0f; }                     // negative and NaN -> 0
__device__ __forceinline__ float invert(float d, float md) { return d > 0.1f ? md - d : d; }
__device__ __forceinline__ int reflect101(int p, int n)
{
    if (p < 0) p = -p;
    if (p >= n) p = 2 * n - 2 - p;
    return min(max(p, 0), n - 1);
}

// One tile of the image with its ring in LDS: R x R floats, local (0,0) is image (oy, ox).
template <int R> struct Tile {
    int oy, ox, H, W;

    // dst[p] = f(ly, lx, y, x) at every position of the region with margin m that lies inside the image
    template <class F> __device__ __forceinline__ void stage(float* dst, int m, F f) const
    {
        const int n = R - 2 * m;
        for (int i = threadIdx.x; i < n * n; i += NT) {
            const int ly = m + i / n, lx = m + i % n;
            const int y = oy + ly, x = ox + lx;
            if (y >= 0 && y < H && x >= 0 && x < W) dst[ly * R + lx] = f(ly, lx, y, x);
        }
        __syncthreads();
    }

    // the interior (margin m) of an LDS buffer -> a [H,W] plane
    __device__ __forceinline__ void store(const float* src, int m, float* plane) const
    {
        const int n = R - 2 * m;
        for (int i = threadIdx.x; i < n * n; i += NT) {
            const int ly = m + i / n, lx = m + i % n;
            const int y = oy + ly, x = ox + lx;
            if (y < H && x < W) plane[(long)y * W + x] = src[ly * R + lx];
        }
    }

    // maximum (MAX) or minimum over the (2r+1)^2 window, taps outside the image ignored
    template <bool MAX> __device__ __forceinline__ float full(const float* src, int ly, int lx, int y, int x, int r) const
    {
        const int a0 = max(-r, -y), a1 = min(r, H - 1 - y), b0 = max(-r, -x), b1 = min(r, W - 1 - x);
        float v = src[ly * R + lx];
        for (int dy = a0; dy <= a1; ++dy)
            for (int dx = b0; dx <= b1; ++dx) {
                const float t = src[(ly + dy) * R + lx + dx];
                v = MAX ? fmaxf(v, t) : fminf(v, t);
            }
        return v;
    }

    // maximum over the 5 x 5 diamond |dy| + |dx| <= 2
    __device__ __forceinline__ float diamond5(const float* src, int ly, int lx, int y, int x) const
    {
        float v = src[ly * R + lx];
        for (int dy = max(-2, -y); dy <= min(2, H - 1 - y); ++dy) {
            const int w = 2 - abs(dy);
            for (int dx = max(-w, -x); dx <= min(w, W - 1 - x); ++dx) v = fmaxf(v, src[(ly + dy) * R + lx + dx]);
        }
        return v;
    }

    // the 13th smallest of the 5 x 5 window, replicated border.  Forgetful selection in registers: of 14 values neither the smallest
    // nor the largest can be the median of 25; drop both, take the next value in, and so on down to three.
    __device__ __forceinline__ float median5(const float* src, int ly, int lx, int y, int x) const
    {
        int ry[5], rx[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            ry[k] = (ly + (min(max(y + k - 2, 0), H - 1) - y)) * R;
            rx[k] = lx + (min(max(x + k - 2, 0), W - 1) - x);
        }
        float v[25];
#pragma unroll
        for (int k = 0; k < 25; ++k) v[k] = src[ry[k / 5] + rx[k % 5]];
        float w[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) w[k] = v[k];
#pragma unroll
        for (int n = 14; n >= 3; --n) {                                    // w[0 .. n-1] are live
#pragma unroll
            for (int i = n - 1; i > 0; --i) {                              // the smallest to w[0]
                const float lo = fminf(w[i - 1], w[i]), hi = fmaxf(w[i - 1], w[i]);
                w[i - 1] = lo; w[i] = hi;
            }
#pragma unroll
            for (int i = 1; i < n - 1; ++i) {                              // the largest to w[n-1]
                const float lo = fminf(w[i], w[i + 1]), hi = fmaxf(w[i], w[i + 1]);
                w[i] = lo; w[i + 1] = hi;
            }
            if (n > 3) w[0] = v[14 + (14 - n)];                            // both dropped, the next one in: w[0 .. n-2] are live
        }
        return w[1];
    }

    // the 13 taps with dx^2 + dy^2 <= 4 in row-major order, reflect-101 border; fp32, one operation at a time
    __device__ __forceinline__ float bilateral(const float* src, int ly, int lx, int y, int x, const Bilateral& bl) const
    {
        const float a = src[ly * R + lx];
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const int row = (ly + (reflect101(y + dy, H) - y)) * R;
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int r2 = dx * dx + dy * dy;
                if (r2 > 4) continue;
                const float v = src[row + lx + (reflect101(x + dx, W) - x)];
                const float dv = v - a;
                const float e = (dv * dv) * bl.cc;
                const float ws = r2 == 0 ? bl.w0 : (r2 == 1 ? bl.w1 : (r2 == 2 ? bl.w2 : bl.w4));
                const float w = ws * expf(e);
                num = num + w * v;
                den = den + w;
            }
        }
        return num / den;
    }
};

__device__ __forceinline__ int top_row(const int* __restrict__ top, int x)
{
    const int r = top[x];
    return r == TOP_NONE ? 0 : r;
}

// ---- multiscale, first launch: s1 .. s4 and the column tops of s4 -------------------------------------------------------------------
constexpr int HEAD_T = 64, HEAD_HALO = 9, HEAD_R = HEAD_T + 2 * HEAD_HALO;

__global__ __launch_bounds__(NT) void fill_ms_head_kernel(const float* __restrict__ depth, int H, int W, float md, float* __restrict__ s4,
                                                          int* __restrict__ top, float* __restrict__ stages, long stage_stride)
{
    constexpr int R = HEAD_R;
    __shared__ float buf0[R * R], buf1[R * R];
    const int b = blockIdx.z;
    const long plane = (long)b * H * W;
    const Tile<R> t = {(int)blockIdx.y * HEAD_T - HEAD_HALO, (int)blockIdx.x * HEAD_T - HEAD_HALO, H, W};
    depth += plane;
    for (int i = threadIdx.x; i < R * R; i += NT) {                        // the cleaned input
        const int y = t.oy + i / R, x = t.ox + i % R;
        buf0[i] = (y >= 0 && y < H && x >= 0 && x < W) ? clean(depth[(long)y * W + x]) : 0.0f;
    }
    __syncthreads();
    // s2: the inverted depth, overwritten by the cross dilations of its far / med / near parts, in that order
    t.stage(buf1, 3, [&](int ly, int lx, int y, int x) {
        float mf = -INFINITY, mm = -INFINITY, mn = -INFINITY;
#pragma unroll
        for (int k = -3; k <= 3; ++k) {
#pragma unroll
            for (int dir = 0; dir < 2; ++dir) {
                if (dir == 1 && k == 0) continue;
                const int yy = y + (dir ? k : 0), xx = x + (dir ? 0 : k);
                if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                const float d = buf0[(ly + (dir ? k : 0)) * R + lx + (dir ? 0 : k)];
                const float s = invert(d, md);
                const bool near = d > 0.1f && d <= 15.0f, med = d > 15.0f && d <= 30.0f, far = d > 30.0f;
                mn = fmaxf(mn, near ? s : 0.0f);
                if (abs(k) <= 2) mm = fmaxf(mm, med ? s : 0.0f);
                if (abs(k) <= 1) mf = fmaxf(mf, far ? s : 0.0f);
            }
        }
        float v = invert(buf0[ly * R + lx], md);
        if (mf > 0.1f) v = mf;
        if (mm > 0.1f) v = mm;
        if (mn > 0.1f) v = mn;
        return v;
    });
    if (stages) {
        float* s1 = stages + plane;
        for (int i = threadIdx.x; i < HEAD_T * HEAD_T; i += NT) {
            const int ly = HEAD_HALO + i / HEAD_T, lx = HEAD_HALO + i % HEAD_T;
            const int y = t.oy + ly, x = t.ox + lx;
            if (y < H && x < W) s1[(long)y * W + x] = invert(buf0[ly * R + lx], md);
        }
        t.store(buf1, HEAD_HALO, stages + stage_stride + plane);
        __syncthreads();                                                   // buf0 is overwritten next
    }
    t.stage(buf0, 5, [&](int ly, int lx, int y, int x) { return t.template full<true>(buf1, ly, lx, y, x, 2); });
    t.stage(buf1, 7, [&](int ly, int lx, int y, int x) { return t.template full<false>(buf0, ly, lx, y, x, 2); });      // s3
    if (stages) t.store(buf1, HEAD_HALO, stages + 2 * stage_stride + plane);
    t.stage(buf0, 9, [&](int ly, int lx, int y, int x) {                                                               // s4
        const float v = buf1[ly * R + lx];
        return v > 0.1f ? t.median5(buf1, ly, lx, y, x) : v;
    });
    t.store(buf0, HEAD_HALO, s4 + plane);
    if (threadIdx.x < HEAD_T) {                                            // one thread per column: its first valid row in this tile
        const int lx = HEAD_HALO + threadIdx.x, x = t.ox + lx;
        if (x < W) {
            const int rows = min(HEAD_T, H - (t.oy + HEAD_HALO));
            for (int j = 0; j < rows; ++j)
                if (buf0[(HEAD_HALO + j) * R + lx] > 0.1f) {
                    atomicMin(&top[(long)b * W + x], t.oy + HEAD_HALO + j);
                    break;
                }
        }
    }
}

// ---- multiscale, second launch: s5 and its column tops ------------------------------------------------------------------------------
// 64 columns x 32 rows per workgroup, a thread walks 8 rows of one column downwards.  Only an empty pixel under the top mask reads its
// 81 taps, from L2.
constexpr int HOLE_ROWS = 32;

__global__ __launch_bounds__(NT) void fill_ms_hole_kernel(const float* __restrict__ s4, const int* __restrict__ top4, int H, int W,
                                                          float* __restrict__ s5, int* __restrict__ top5)
{
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    if (x >= W) return;
    const long plane = (long)b * H * W;
    s4 += plane;
    s5 += plane;
    const int r0 = top_row(top4 + (long)b * W, x);
    const int y0 = blockIdx.y * HOLE_ROWS + (threadIdx.x >> 6) * 8;
    int first = -1;
    for (int y = y0; y < min(y0 + 8, H); ++y) {
        float v = s4[(long)y * W + x];
        if (!(v > 0.1f) && y >= r0) {
            for (int yy = max(y - 4, 0); yy <= min(y + 4, H - 1); ++yy)
                for (int xx = max(x - 4, 0); xx <= min(x + 4, W - 1); ++xx) v = fmaxf(v, s4[(long)yy * W + xx]);
        }
        s5[(long)y * W + x] = v;
        if (first < 0 && v > 0.1f) first = y;
    }
    if (first >= 0) atomicMin(&top5[(long)b * W + x], first);
}

// ---- multiscale, third launch: the six masked dilations, median, bilateral, inversion -----------------------------------------------
constexpr int TAIL_T = 48, TAIL_HALO = 16, TAIL_R = TAIL_T + 2 * TAIL_HALO;

__global__ __launch_bounds__(NT) void fill_ms_tail_kernel(const float* __restrict__ s5, const int* __restrict__ top5, int H, int W, float md,
                                                          Bilateral bl, float* __restrict__ out, float* __restrict__ stages,
                                                          long stage_stride)
{
    constexpr int R = TAIL_R;
    __shared__ float buf0[R * R], buf1[R * R];
    __shared__ int r0s[R];
    const int b = blockIdx.z;
    const long plane = (long)b * H * W;
    const Tile<R> t = {(int)blockIdx.y * TAIL_T - TAIL_HALO, (int)blockIdx.x * TAIL_T - TAIL_HALO, H, W};
    s5 += plane;
    for (int i = threadIdx.x; i < R * R; i += NT) {
        const int y = t.oy + i / R, x = t.ox + i % R;
        buf0[i] = (y >= 0 && y < H && x >= 0 && x < W) ? s5[(long)y * W + x] : 0.0f;
    }
    if (threadIdx.x < R) {
        const int x = t.ox + threadIdx.x;
        r0s[threadIdx.x] = (x >= 0 && x < W) ? top_row(top5 + (long)b * W, x) : 0;
    }
    __syncthreads();
    float *src = buf0, *dst = buf1;
#pragma unroll 1
    for (int it = 1; it <= 6; ++it) {
        t.stage(dst, 2 * it, [&](int ly, int lx, int y, int x) {
            const float v = src[ly * R + lx];
            return (v < 0.1f && y >= r0s[lx]) ? t.template full<true>(src, ly, lx, y, x, 2) : v;
        });
        float* s = src; src = dst; dst = s;
    }
    // src == buf0 holds s7 before the median; the same `valid` gates the median and the bilateral
    t.stage(buf1, 14, [&](int ly, int lx, int y, int x) {
        const float v = buf0[ly * R + lx];
        return (v > 0.1f && y >= r0s[lx]) ? t.median5(buf0, ly, lx, y, x) : v;
    });
    if (stages) t.store(buf1, TAIL_HALO, stages + 5 * stage_stride + plane);
    for (int i = threadIdx.x; i < TAIL_T * TAIL_T; i += NT) {
        const int ly = TAIL_HALO + i / TAIL_T, lx = TAIL_HALO + i % TAIL_T;
        const int y = t.oy + ly, x = t.ox + lx;
        if (y >= H || x >= W) continue;
        float v = buf1[ly * R + lx];
        if (buf0[ly * R + lx] > 0.1f && y >= r0s[lx]) v = t.bilateral(buf1, ly, lx, y, x, bl);
        const long o = plane + (long)y * W + x;
        if (stages) stages[6 * stage_stride + o] = v;
        out[o] = invert(v, md);
    }
}

// ---- fast: the whole operator in one launch -----------------------------------------------------------------------------------------
constexpr int FAST_T = 48, FAST_HALO = 13, FAST_R = FAST_T + 2 * FAST_HALO;

__global__ __launch_bounds__(NT) void fill_fast_kernel(const float* __restrict__ depth, int H, int W, float md, Bilateral bl,
                                                       float* __restrict__ out, float* __restrict__ stages, long stage_stride)
{
    constexpr int R = FAST_R;
    __shared__ float buf0[R * R], buf1[R * R];
    const int b = blockIdx.z;
    const long plane = (long)b * H * W;
    const Tile<R> t = {(int)blockIdx.y * FAST_T - FAST_HALO, (int)blockIdx.x * FAST_T - FAST_HALO, H, W};
    depth += plane;
    for (int i = threadIdx.x; i < R * R; i += NT) {                        // s1
        const int y = t.oy + i / R, x = t.ox + i % R;
        buf0[i] = (y >= 0 && y < H && x >= 0 && x < W) ? invert(clean(depth[(long)y * W + x]), md) : 0.0f;
    }
    __syncthreads();
    if (stages) t.store(buf0, FAST_HALO, stages + plane);
    t.stage(buf1, 2, [&](int ly, int lx, int y, int x) { return t.diamond5(buf0, ly, lx, y, x); });                    // s2
    if (stages) t.store(buf1, FAST_HALO, stages + stage_stride + plane);
    t.stage(buf0, 4, [&](int ly, int lx, int y, int x) { return t.template full<true>(buf1, ly, lx, y, x, 2); });
    t.stage(buf1, 6, [&](int ly, int lx, int y, int x) { return t.template full<false>(buf0, ly, lx, y, x, 2); });     // s3
    if (stages) t.store(buf1, FAST_HALO, stages + 2 * stage_stride + plane);
    t.stage(buf0, 9, [&](int ly, int lx, int y, int x) {                                                               // s5
        const float v = buf1[ly * R + lx];
        return v < 0.1f ? t.template full<true>(buf1, ly, lx, y, x, 3) : v;
    });
    if (stages) t.store(buf0, FAST_HALO, stages + 4 * stage_stride + plane);
    t.stage(buf1, 11, [&](int ly, int lx, int y, int x) { return t.median5(buf0, ly, lx, y, x); });
    if (stages) t.store(buf1, FAST_HALO, stages + 5 * stage_stride + plane);
    for (int i = threadIdx.x; i < FAST_T * FAST_T; i += NT) {
        const int ly = FAST_HALO + i / FAST_T, lx = FAST_HALO + i % FAST_T;
        const int y = t.oy + ly, x = t.ox + lx;
        if (y >= H || x >= W) continue;
        const float v = t.bilateral(buf1, ly, lx, y, x, bl);
        const long o = plane + (long)y * W + x;
        if (stages) stages[6 * stage_stride + o] = v;
        out[o] = invert(v, md);
    }
}

Bilateral make_bilateral(double sigma_color, double sigma_space)
{
    const double g = -0.5 / (sigma_space * sigma_space);
    return {(float)(-0.5 / (sigma_color * sigma_color)), (float)exp(0.0 * g), (float)exp(1.0 * g), (float)exp(2.0 * g),
            (float)exp(4.0 * g)};
}

size_t align256(size_t n) { return (n + 255) / 256 * 256; }

bool shape_ok(int B, int H, int W, int mode)
{
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && (mode == GDM_FILL_MULTISCALE || mode == GDM_FILL_FAST);
}

} // namespace

extern "C" size_t gdm_fill_depth_workspace_bytes(int B, int H, int W, int mode)
{
    if (!shape_ok(B, H, W, mode)) return 0;
    if (mode == GDM_FILL_FAST) return 0;
    return align256(2 * (size_t)B * W * sizeof(int)) + 2 * (size_t)B * H * W * sizeof(float);       // two top tables, s4 and s5
}

extern "C" int gdm_fill_depth_hip(const float* depth, int B, int H, int W, int mode, float max_depth, void* workspace,
                                  size_t workspace_bytes, float* out, float* stages, void* stream)
{
    GDM_CHECK_ARG(depth && out, "gdm_fill_depth_hip: NULL pointer");
    GDM_CHECK_ARG(shape_ok(B, H, W, mode), "gdm_fill_depth_hip: bad shape B=%d H=%d W=%d or mode=%d", B, H, W, mode);
    GDM_CHECK_ARG(max_depth == max_depth, "gdm_fill_depth_hip: max_depth is NaN");
    const size_t need = gdm_fill_depth_workspace_bytes(B, H, W, mode);
    GDM_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need), "gdm_fill_depth_hip: workspace %p of %zu bytes, %zu needed",
                  workspace, workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const long stride = (long)B * H * W;
    if (mode == GDM_FILL_FAST) {
        hipLaunchKernelGGL(fill_fast_kernel, dim3(gdm_cdiv(W, FAST_T), gdm_cdiv(H, FAST_T), B), dim3(NT), 0, s, depth, H, W, max_depth,
                           make_bilateral(1.5, 2.0), out, stages, stride);
        return gdm_launch_status("fill_fast_kernel");
    }
    const size_t tops = 2 * (size_t)B * W * sizeof(int);
    int* top4 = (int*)workspace;
    int* top5 = top4 + (size_t)B * W;
    float* s4 = (float*)((char*)workspace + align256(tops));
    float* s5 = s4 + stride;
    if (stages) { s4 = stages + 3 * stride; s5 = stages + 4 * stride; }
    GDM_HIP(hipMemsetAsync(workspace, 0x7f, tops, s));
    hipLaunchKernelGGL(fill_ms_head_kernel, dim3(gdm_cdiv(W, HEAD_T), gdm_cdiv(H, HEAD_T), B), dim3(NT), 0, s, depth, H, W, max_depth, s4,
                       top4, stages, stride);
    int rc = gdm_launch_status("fill_ms_head_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(fill_ms_hole_kernel, dim3(gdm_cdiv(W, 64), gdm_cdiv(H, HOLE_ROWS), B), dim3(NT), 0, s, s4, top4, H, W, s5, top5);
    rc = gdm_launch_status("fill_ms_hole_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(fill_ms_tail_kernel, dim3(gdm_cdiv(W, TAIL_T), gdm_cdiv(H, TAIL_T), B), dim3(NT), 0, s, s5, top5, H, W, max_depth,
                       make_bilateral(0.5, 2.0), out, stages, stride);
    return gdm_launch_status("fill_ms_tail_kernel");
}
