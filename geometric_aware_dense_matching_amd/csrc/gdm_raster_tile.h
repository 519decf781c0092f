// The LDS tile of gdm_verify.hip and gdm_refine.hip, once: an instance's window clamped to the frame, the kTile x kTile tile of it
// that a workgroup owns, the z-buffer of that tile filled by the drawing loop of gdm_raster.h, and the refusals the two entries share.
// kTile = 64 is 16 KiB of 32-bit keys or 32 KiB of 64-bit ones, so several workgroups fit the 160 KiB of a CU beside each other and a
// 128 x 128 window is four tiles.  (32 would quadruple the tiles, each of which walks all F faces; 128 is 64 KiB of 32-bit keys and one
// workgroup for the whole window, which leaves most CUs idle at 16 x 8 candidates.)
#pragma once
#include "gdm_raster.h"

constexpr int kTile = 64;                                                  // pixels per tile side; kTile^2 keys of LDS

struct Win { int x0, y0, x1, y1; };                                        // inclusive, frame pixels; empty when x0 > x1 or y0 > y1
struct TileBox { int x0, y0, x1, y1; };                                    // inclusive, frame pixels

// The window of instance i clamped to the frame; the whole frame without `window`.
__device__ __forceinline__ Win clamped_window(const int32_t* __restrict__ window, int i, int H, int W)
{
    Win w = {0, 0, W - 1, H - 1};
    if (window) {
        w.x0 = max(window[(long)i * 4], 0);
        w.y0 = max(window[(long)i * 4 + 1], 0);
        w.x1 = min(window[(long)i * 4 + 2], W - 1);
        w.y1 = min(window[(long)i * 4 + 3], H - 1);
    }
    return w;
}

// Tile `block` of window w, the tiles counted from the window's corner, cdiv(W, kTile) to a row: false when the window is empty or
// does not reach that tile.  The same for every thread of a workgroup, so the caller's early return is uniform; it comes before any
// LDS access.  The tiles that exist are those with tx <= (w.x1 - w.x0) / kTile and ty <= (w.y1 - w.y0) / kTile.
__device__ __forceinline__ bool tile_of_block(const Win& w, int block, int W, TileBox& t)
{
    if (w.x0 > w.x1 || w.y0 > w.y1) return false;
    const int tiles_x = (W + kTile - 1) / kTile;
    t.x0 = w.x0 + (block % tiles_x) * kTile;                               // w.x0 < W <= 16384: no overflow
    t.y0 = w.y0 + (block / tiles_x) * kTile;
    if (t.x0 > w.x1 || t.y0 > w.y1) return false;
    t.x1 = min(t.x0 + kTile - 1, w.x1);
    t.y1 = min(t.y0 + kTile - 1, w.y1);
    return true;
}

// Clears the tile's z-buffer zt[kTile * kTile] to all-ones and draws all F faces into it, THREADS at a time: set-up with the frame's
// H, W, the pixel box then clamped to the tile (and with it to window and frame), shade on the key type K.  Every thread of the
// workgroup calls it; it ends at the barrier after which zt holds the tile.
template <int THREADS, typename K, typename VT>
__device__ __forceinline__ void draw_tile(K* zt, const TileBox& t, const VT* __restrict__ verts, const int32_t* __restrict__ faces,
                                          int V, int F, const double* __restrict__ rt, const double* __restrict__ kk, double near, int H,
                                          int W)
{
    for (int k = threadIdx.x; k < kTile * kTile; k += THREADS) zt[k] = ~(K)0;
    __syncthreads();
    for (int base = 0; base < F; base += THREADS) {                        // uniform trip count: every lane reaches the ballot
        const int f = base + (int)threadIdx.x;
        TriSetup s = {};
        bool valid = f < F;
        if (valid) {
            bool swapped;
            valid = tri_setup(verts, V, faces[(long)f * 3], faces[(long)f * 3 + 1], faces[(long)f * 3 + 2], rt, kk, near, H, W, s, swapped);
        }
        if (valid) {
            s.px0 = max(s.px0, t.x0); s.px1 = min(s.px1, t.x1);
            s.py0 = max(s.py0, t.y0); s.py1 = min(s.py1, t.y1);
            valid = s.px0 <= s.px1 && s.py0 <= s.py1;
        }
        draw_wave_triangles(s, valid, (unsigned)f, [=](unsigned face, int px, int py, unsigned bits) {
            shade(&zt[(py - t.y0) * kTile + (px - t.x0)], bits, face);
        });
    }
    __syncthreads();
}

// The refusals gdm_pose_verify_hip and gdm_pose_refine_depth_hip share, under the entry's name `me`; `px_why` ends the sentence about
// 2^22 pixels.  The grid is (tiles, C, n) with every tile a window can have.
static inline int tile_entry_check(const char* me, const char* px_why, int n, int C, int V, int F, int H, int W, double near,
                                   int k_per_instance, int obs_per_instance, int verts_f64)
{
    GDM_CHECK_ARG(n >= 1 && n <= 65535 && C >= 1 && C <= 65535, "%s: n=%d C=%d not in [1, 65535]", me, n, C);
    GDM_CHECK_ARG(V >= 1 && F >= 1, "%s: V=%d F=%d must be positive", me, V, F);
    GDM_CHECK_ARG(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "%s: H=%d W=%d not in [1, 16384]", me, H, W);
    GDM_CHECK_ARG((long)H * W <= (1L << 22), "%s: H=%d W=%d: more than 2^22 pixels%s", me, H, W, px_why);
    const long tiles = (long)gdm_cdiv(W, kTile) * gdm_cdiv(H, kTile);       // at most 256 * 256
    GDM_CHECK_ARG(tiles * n * C <= (1L << 23), "%s: n=%d C=%d too large for H=%d W=%d (tiles n C <= 2^23)", me, n, C, H, W);
    GDM_CHECK_ARG(near >= 0.0, "%s: near=%g must be >= 0", me, near);
    GDM_CHECK_ARG(k_per_instance == 0 || k_per_instance == 1, "%s: k_per_instance=%d must be 0 or 1", me, k_per_instance);
    GDM_CHECK_ARG(obs_per_instance == 0 || obs_per_instance == 1, "%s: obs_per_instance=%d must be 0 or 1", me, obs_per_instance);
    GDM_CHECK_ARG(verts_f64 == 0 || verts_f64 == 1, "%s: verts_f64=%d must be 0 or 1", me, verts_f64);
    return 0;
}
