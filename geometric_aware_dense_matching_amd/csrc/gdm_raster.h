// The one copy of the pixel rule of include/gdm.h (gdm_render_depth_hip) and of the wave's drawing loop, shared by the
// depth rasteriser of gdm_bop.hip, the frame renderer of gdm_render.hip and, through gdm_raster_tile.h, the LDS tiles of gdm_verify.hip
// and gdm_refine.hip: fp64 vertex transform and projection, discard, snapping to 1/256 px, int64 edge functions with the top-left
// rule, the winding normalised by the sign of the snapped area, the pixel box clamped to the image (tri_setup); then
// draw_wave_triangles, which walks a small box with the owning lane and draws a larger one with all 64 lanes, and shade, the
// atomicMin of the depth key that every z-buffer of the family keeps, in LDS or in memory.
#pragma once
#include "gdm_common.h"

constexpr int kSmallBox = 64;                                              // pixels a single thread may walk for one triangle

struct TriSetup {
    int x0, y0, x1, y1, x2, y2;                                            // snapped vertices (1/256 px), normalised winding
    double iz0, iz1, iz2;                                                  // 1 / z of the vertices
    int px0, px1, py0, py1;                                                // clamped pixel box, inclusive
};

__device__ __forceinline__ long long edge_fn(int ax, int ay, int bx, int by, long long X, long long Y)
{
    return (long long)(bx - ax) * (Y - ay) - (long long)(by - ay) * (X - ax);
}

__device__ __forceinline__ bool edge_in(long long w, int dx, int dy) { return w > 0 || (w == 0 && (dy < 0 || (dy == 0 && dx > 0))); }

// The three edge values of s at pixel (px, py), w_i opposite vertex i; false when the pixel is not covered.
__device__ __forceinline__ bool edge_values(const TriSetup& s, int px, int py, long long& w0, long long& w1, long long& w2)
{
    const long long X = (long long)px * 256, Y = (long long)py * 256;
    w0 = edge_fn(s.x1, s.y1, s.x2, s.y2, X, Y);                            // opposite vertex 0
    w1 = edge_fn(s.x2, s.y2, s.x0, s.y0, X, Y);
    w2 = edge_fn(s.x0, s.y0, s.x1, s.y1, X, Y);
    return edge_in(w0, s.x2 - s.x1, s.y2 - s.y1) && edge_in(w1, s.x0 - s.x2, s.y0 - s.y2) && edge_in(w2, s.x1 - s.x0, s.y1 - s.y0);
}

// The depth of a covered pixel from its edge values.
__device__ __forceinline__ float pixel_depth(const TriSetup& s, long long w0, long long w1, long long w2)
{
    const double A = (double)((w0 + w1) + w2);
    const double iz = (((double)w0 * s.iz0 + (double)w1 * s.iz1) + (double)w2 * s.iz2) / A;
    return (float)(1.0 / iz);
}

__device__ __forceinline__ bool project_vertex(const double* __restrict__ rt, double fx, double fy, double cx, double cy, double near,
                                               double x, double y, double z, int& xs, int& ys, double& iz)
{
    const double X = ((rt[0] * x + rt[1] * y) + rt[2] * z) + rt[3];
    const double Y = ((rt[4] * x + rt[5] * y) + rt[6] * z) + rt[7];
    const double Z = ((rt[8] * x + rt[9] * y) + rt[10] * z) + rt[11];
    if (!(Z > near)) return false;
    const double u = fx * (X / Z) + cx, v = fy * (Y / Z) + cy;
    if (!(fabs(u) <= 65536.0) || !(fabs(v) <= 65536.0)) return false;
    xs = (int)(long long)floor(u * 256.0 + 0.5);
    ys = (int)(long long)floor(v * 256.0 + 0.5);
    iz = 1.0 / Z;
    return true;
}

// The set-up of the triangle (i0, i1, i2) of verts[V,3] under the pose rt[3,4] and the intrinsics kk[3,3]: false when the rule
// discards it (an index outside [0, V), a vertex behind `near` or off the snapping range, a snapped area of 0, an empty clamped box).
// `swapped` says that vertices 1 and 2 changed places to normalise the winding: whoever interpolates attributes swaps them too.
template <typename VT>
__device__ __forceinline__ bool tri_setup(const VT* __restrict__ verts, int V, int i0, int i1, int i2, const double* __restrict__ rt,
                                          const double* __restrict__ kk, double near, int H, int W, TriSetup& s, bool& swapped)
{
    swapped = false;
    if (!(i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V)) return false;
    const double fx = kk[0], fy = kk[4], cx = kk[2], cy = kk[5];
    bool valid = project_vertex(rt, fx, fy, cx, cy, near, (double)verts[(long)i0 * 3], (double)verts[(long)i0 * 3 + 1],
                                (double)verts[(long)i0 * 3 + 2], s.x0, s.y0, s.iz0);
    valid = project_vertex(rt, fx, fy, cx, cy, near, (double)verts[(long)i1 * 3], (double)verts[(long)i1 * 3 + 1],
                           (double)verts[(long)i1 * 3 + 2], s.x1, s.y1, s.iz1) && valid;
    valid = project_vertex(rt, fx, fy, cx, cy, near, (double)verts[(long)i2 * 3], (double)verts[(long)i2 * 3 + 1],
                           (double)verts[(long)i2 * 3 + 2], s.x2, s.y2, s.iz2) && valid;
    if (!valid) return false;
    const long long A2 = (long long)(s.x1 - s.x0) * (s.y2 - s.y0) - (long long)(s.x2 - s.x0) * (s.y1 - s.y0);
    if (A2 == 0) return false;
    if (A2 < 0) {                                                          // normalise the winding: both are drawn
        const int tx = s.x1, ty = s.y1;
        const double tz = s.iz1;
        s.x1 = s.x2; s.y1 = s.y2; s.iz1 = s.iz2;
        s.x2 = tx; s.y2 = ty; s.iz2 = tz;
        swapped = true;
    }
    const int xmin = min(s.x0, min(s.x1, s.x2)), xmax = max(s.x0, max(s.x1, s.x2));
    const int ymin = min(s.y0, min(s.y1, s.y2)), ymax = max(s.y0, max(s.y1, s.y2));
    s.px0 = max((xmin + 255) >> 8, 0);
    s.px1 = min(xmax >> 8, W - 1);
    s.py0 = max((ymin + 255) >> 8, 0);
    s.py1 = min(ymax >> 8, H - 1);
    return s.px0 <= s.px1 && s.py0 <= s.py1;
}

// A triangle set-up of lane `src`, for the whole wave.
__device__ __forceinline__ TriSetup tri_from_lane(const TriSetup& s, int src)
{
    TriSetup c;
    c.x0 = __shfl(s.x0, src, 64); c.y0 = __shfl(s.y0, src, 64);
    c.x1 = __shfl(s.x1, src, 64); c.y1 = __shfl(s.y1, src, 64);
    c.x2 = __shfl(s.x2, src, 64); c.y2 = __shfl(s.y2, src, 64);
    c.iz0 = __shfl(s.iz0, src, 64); c.iz1 = __shfl(s.iz1, src, 64); c.iz2 = __shfl(s.iz2, src, 64);
    c.px0 = __shfl(s.px0, src, 64); c.px1 = __shfl(s.px1, src, 64);
    c.py0 = __shfl(s.py0, src, 64); c.py1 = __shfl(s.py1, src, 64);
    return c;
}

// A small plain-data payload of lane `src`, for the whole wave: one __shfl per 32-bit word.
struct NoPayload {};

template <typename P>
__device__ __forceinline__ P payload_from_lane(const P& p, int src)
{
    if constexpr (std::is_empty<P>::value) {
        return p;
    } else {
        static_assert(std::is_trivially_copyable<P>::value && sizeof(P) % sizeof(int) == 0, "a payload is whole words of plain data");
        int w[sizeof(P) / sizeof(int)];
        __builtin_memcpy(w, &p, sizeof(P));
#pragma unroll
        for (unsigned k = 0; k < sizeof(P) / sizeof(int); ++k) w[k] = __shfl(w[k], src, 64);
        P c;
        __builtin_memcpy(&c, w, sizeof(P));
        return c;
    }
}

// The drawing loop of a wave.  Every lane of the wave must call it (it ballots), each with the set-up of its own triangle, `valid`
// false where it has none, and the payload its sink needs to find the buffer and name the face.  A box of at most kSmallBox pixels is
// walked by the owning lane; the larger ones are drawn one after the other by all 64 lanes, set-up and payload broadcast from the
// source lane once per triangle.  sink(payload, px, py, bits) gets every covered pixel and the fp32 bits of its depth.  A clamped box
// holds at most 16384^2 = 2^28 pixels (the entries refuse a larger H or W): int counts it.
template <typename P, typename Sink>
__device__ __forceinline__ void draw_wave_triangles(const TriSetup& s, bool valid, const P& payload, Sink sink)
{
    const int lane = threadIdx.x & 63;
    const int box = valid ? (s.px1 - s.px0 + 1) * (s.py1 - s.py0 + 1) : 0;
    long long w0, w1, w2;
    if (valid && box <= kSmallBox) {
        for (int py = s.py0; py <= s.py1; ++py)
            for (int px = s.px0; px <= s.px1; ++px)
                if (edge_values(s, px, py, w0, w1, w2)) sink(payload, px, py, __float_as_uint(pixel_depth(s, w0, w1, w2)));
    }
    unsigned long long big = __ballot(valid && box > kSmallBox);
    while (big) {
        const int src = __ffsll((long long)big) - 1;
        big &= big - 1;
        const TriSetup c = tri_from_lane(s, src);
        const P cp = payload_from_lane(payload, src);
        const int bw = c.px1 - c.px0 + 1;
        const int cnt = bw * (c.py1 - c.py0 + 1);
        for (int k = lane; k < cnt; k += 64) {
            const int px = c.px0 + k % bw, py = c.py0 + k / bw;
            if (edge_values(c, px, py, w0, w1, w2)) sink(cp, px, py, __float_as_uint(pixel_depth(c, w0, w1, w2)));
        }
    }
}

// The z-buffer's one operation: the unsigned minimum of the key at p, in LDS or in memory.  A 32-bit key is the fp32 depth bits
// (positive floats order like their bits); a 64-bit key is bits << 32 | face, so equal depths go to the lower face.  A minimum over
// integers does not depend on arrival order.
template <typename K>
__device__ __forceinline__ void shade(K* p, unsigned bits, unsigned face)
{
    if constexpr (sizeof(K) == sizeof(unsigned))
        atomicMin(p, bits);
    else
        atomicMin(p, ((K)bits << 32) | face);
}
