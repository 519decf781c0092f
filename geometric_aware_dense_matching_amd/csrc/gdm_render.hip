// Training frames from triangle meshes on the device, gfx950: colour, depth, instance mask, face ids and the per-slot visibility
// statistics of n frames of up to GDM_RENDER_MAX_SLOTS posed objects each, by the written rule of include/gdm.h
// (gdm_render_frames_hip; render.render_frames_numpy restates it bit for bit, drawing with pixel_rule.py).  Coverage
// and depth are the pixel rule of gdm_render_depth_hip, from its one copy in gdm_raster.h, and so is the wave's drawing loop.
//   clear_kernel     the slot layers to all-ones and the statistics to (0, 0, W, H, -1, -1).  A kernel, not hipMemsetAsync: see the
//                    header comment of gdm_bop.hip for what the runtime's memset node did under graph replay.
//   vis_kernel       one thread per (frame, slot, face of the slot's object), drawn by draw_wave_triangles of gdm_raster.h with the
//                    payload (slot, face): a triangle whose clamped box holds more than kSmallBox pixels is drawn by its whole wave,
//                    as raster_kernel does.  Every covered pixel does ONE 64-bit unsigned atomicMin
//                    (global_atomic_umin_x2, no compare-and-swap loop) of (fp32 depth bits << 32 | global face id) into its slot's
//                    layer: a minimum over integers does not depend on arrival order, and equal depths go to the lower face id.
//   resolve_kernel   one thread per pixel: the winning slot (smallest depth bits, the lower slot on a tie), the set-up of the winning
//                    face once more, perspective-correct colour and normal in fp64, the diffuse term, and the statistics -- counted by
//                    ballot and reduced by shuffles per wave, then one integer atomic per wave and counter that has something to say
//                    (integer adds, minima and maxima are order-independent).
// No allocation and no host read in the entry point: it captures in a hipGraph.
#include "gdm_common.h"
#include "gdm_raster.h"

namespace {

constexpr int kThreads = 256;
typedef unsigned long long u64;
constexpr u64 kEmptyKey = ~0ull;

struct ObjTable { int32_t face0[GDM_RENDER_MAX_OBJECTS + 1]; };            // the objects' face ranges, by value in the kernel arguments

__global__ __launch_bounds__(kThreads) void clear_kernel(u64* __restrict__ keys, long count, int32_t* __restrict__ stats, int slots,
                                                         int H, int W)
{
    const long t0 = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
    for (long i = t0; i < count; i += step) keys[i] = kEmptyKey;
    for (long i = t0; i < slots; i += step) {
        int32_t* st = stats + i * 6;
        st[0] = 0; st[1] = 0; st[2] = W; st[3] = H; st[4] = -1; st[5] = -1;
    }
}

struct SlotFace { int slot, face; };                                       // b * S + s and the global face id

template <typename VT>
__global__ __launch_bounds__(kThreads) void vis_kernel(const VT* __restrict__ verts, const int32_t* __restrict__ faces,
                                                       const int32_t* __restrict__ slot_obj, const ObjTable tab, int O,
                                                       const double* __restrict__ RT, const double* __restrict__ Kmat, int k_per_instance,
                                                       int n, int S, int Vt, int Fmax, int H, int W, double near, u64* __restrict__ keys)
{
    const long gid = (long)blockIdx.x * kThreads + threadIdx.x;
    TriSetup s = {};
    bool valid = gid < (long)n * S * Fmax;
    long slot = 0;                                                         // b * S + s
    int f = 0;
    if (valid) {
        slot = gid / Fmax;
        const int local = (int)(gid % Fmax);
        const int o = slot_obj[slot];
        valid = o >= 0 && o < O;                                           // an empty slot, or an index the table does not hold
        if (valid) {
            f = tab.face0[o] + local;
            valid = f < tab.face0[o + 1];
        }
        if (valid) {
            const int b = (int)(slot / S);
            bool swapped;
            valid = tri_setup(verts, Vt, faces[(long)f * 3], faces[(long)f * 3 + 1], faces[(long)f * 3 + 2], RT + slot * 12,
                              Kmat + (k_per_instance ? (long)b * 9 : 0), near, H, W, s, swapped);
        }
    }
    draw_wave_triangles(s, valid, SlotFace{(int)slot, f}, [=](SlotFace c, int px, int py, unsigned bits) {       // slot < n S <= 2^30
        shade(&keys[(long)c.slot * H * W + (long)py * W + px], bits, (unsigned)c.face);
    });
}

__device__ __forceinline__ int wave_min_i32(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ int wave_max_i32(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// ((q0 a0 + q1 a1) + q2 a2) / Q
__device__ __forceinline__ double interp(double q0, double q1, double q2, double Q, double a0, double a1, double a2)
{
    return ((q0 * a0 + q1 * a1) + q2 * a2) / Q;
}

template <typename VT>
__global__ __launch_bounds__(kThreads) void resolve_kernel(const VT* __restrict__ verts, const uint8_t* __restrict__ vcol,
                                                           const float* __restrict__ vnrm, const int32_t* __restrict__ faces,
                                                           const double* __restrict__ RT, const double* __restrict__ Kmat,
                                                           int k_per_instance, const double* __restrict__ light, double ambient, double near,
                                                           int S, int Vt, int Ft, int H, int W, const u64* __restrict__ keys,
                                                           uint8_t* __restrict__ rgb, float* __restrict__ depth, uint8_t* __restrict__ inst,
                                                           int32_t* __restrict__ face, int32_t* __restrict__ stats)
{
    const int b = blockIdx.y;
    const long P = (long)H * W;
    const long p = (long)blockIdx.x * kThreads + threadIdx.x;
    const bool in = p < P;
    const int px = in ? (int)(p % W) : 0, py = in ? (int)(p / W) : 0;
    const int lane = threadIdx.x & 63;
    u64 best = kEmptyKey;
    int win = -1;
    unsigned has = 0;
    if (in) {
        for (int s = 0; s < S; ++s) {
            const u64 k = keys[((long)b * S + s) * P + p];
            if (k != kEmptyKey) has |= 1u << s;
            if ((unsigned)(k >> 32) < (unsigned)(best >> 32)) {            // strictly nearer: the lower slot keeps a tie
                best = k;
                win = s;
            }
        }
        int r = 0, g = 0, bl = 0;
        if (win >= 0) {
            const int f = (int)(unsigned)(best & 0xffffffffu);
            int i0 = 0, i1 = 0, i2 = 0;
            TriSetup t = {};
            bool swapped = false, ok = f >= 0 && f < Ft;
            if (ok) {
                i0 = faces[(long)f * 3]; i1 = faces[(long)f * 3 + 1]; i2 = faces[(long)f * 3 + 2];
                ok = tri_setup(verts, Vt, i0, i1, i2, RT + ((long)b * S + win) * 12, Kmat + (k_per_instance ? (long)b * 9 : 0), near, H, W,
                               t, swapped);
            }
            long long w0 = 0, w1 = 0, w2 = 0;
            ok = ok && edge_values(t, px, py, w0, w1, w2);                 // pass 1 drew this pixel from this face: it holds
            if (ok) {
                if (swapped) { const int tmp = i1; i1 = i2; i2 = tmp; }    // the attributes follow the winding
                const double q0 = (double)w0 * t.iz0, q1 = (double)w1 * t.iz1, q2 = (double)w2 * t.iz2;
                const double Q = (q0 + q1) + q2;
                const uint8_t* c0 = vcol + (long)i0 * 3;
                const uint8_t* c1 = vcol + (long)i1 * 3;
                const uint8_t* c2 = vcol + (long)i2 * 3;
                const float* n0 = vnrm + (long)i0 * 3;
                const float* n1 = vnrm + (long)i1 * 3;
                const float* n2 = vnrm + (long)i2 * 3;
                const double ox = interp(q0, q1, q2, Q, (double)n0[0], (double)n1[0], (double)n2[0]);
                const double oy = interp(q0, q1, q2, Q, (double)n0[1], (double)n1[1], (double)n2[1]);
                const double oz = interp(q0, q1, q2, Q, (double)n0[2], (double)n1[2], (double)n2[2]);
                const double* rt = RT + ((long)b * S + win) * 12;
                const double nx = (rt[0] * ox + rt[1] * oy) + rt[2] * oz;
                const double ny = (rt[4] * ox + rt[5] * oy) + rt[6] * oz;
                const double nz = (rt[8] * ox + rt[9] * oy) + rt[10] * oz;
                const double len = sqrt((nx * nx + ny * ny) + nz * nz);
                const double* l = light + (long)b * 3;
                const double cs = len > 0.0 ? fmax(((nx * l[0] + ny * l[1]) + nz * l[2]) / len, 0.0) : 0.0;
                const double k = ambient + (1.0 - ambient) * cs;
                r = (int)fmin(255.0, floor(interp(q0, q1, q2, Q, (double)c0[0], (double)c1[0], (double)c2[0]) * k + 0.5));
                g = (int)fmin(255.0, floor(interp(q0, q1, q2, Q, (double)c0[1], (double)c1[1], (double)c2[1]) * k + 0.5));
                bl = (int)fmin(255.0, floor(interp(q0, q1, q2, Q, (double)c0[2], (double)c1[2], (double)c2[2]) * k + 0.5));
            }
        }
        const long o = (long)b * P + p;
        rgb[o * 3] = (uint8_t)r; rgb[o * 3 + 1] = (uint8_t)g; rgb[o * 3 + 2] = (uint8_t)bl;
        depth[o] = win >= 0 ? __uint_as_float((unsigned)(best >> 32)) : 0.f;
        inst[o] = (uint8_t)(win + 1);
        face[o] = win >= 0 ? (int)(unsigned)(best & 0xffffffffu) : -1;
    }
    // statistics: every lane of the wave reaches this point; the branches below are taken by whole waves
    for (int s = 0; s < S; ++s) {
        const u64 all = __ballot((has >> s) & 1u);
        const bool mine = win == s;
        const u64 vis = __ballot(mine);
        int32_t* st = stats + ((long)b * S + s) * 6;
        if (all && lane == 0) atomicAdd(&st[0], __popcll(all));
        if (vis) {
            const int x0 = wave_min_i32(mine ? px : 0x7fffffff), y0 = wave_min_i32(mine ? py : 0x7fffffff);
            const int x1 = wave_max_i32(mine ? px : -1), y1 = wave_max_i32(mine ? py : -1);
            if (lane == 0) {
                atomicAdd(&st[1], __popcll(vis));
                atomicMin(&st[2], x0); atomicMin(&st[3], y0);
                atomicMax(&st[4], x1); atomicMax(&st[5], y1);
            }
        }
    }
}

} // namespace

extern "C" size_t gdm_render_frames_workspace_bytes(int n, int S, int H, int W)
{
    if (n < 1 || n > 65535 || S < 1 || S > GDM_RENDER_MAX_SLOTS || H < 1 || H > 16384 || W < 1 || W > 16384) return 0;
    return (size_t)n * S * H * W * sizeof(u64);
}

extern "C" int gdm_render_frames_hip(const void* verts, int verts_f64, const uint8_t* vcol, const float* vnrm, const int32_t* faces,
                                     const int32_t* obj_face0, const int32_t* slot_obj, const double* RT, const double* K,
                                     int k_per_instance, const double* light, double ambient, double near, int n, int S, int O, int Vt,
                                     int Ft, int H, int W, void* workspace, size_t workspace_bytes, uint8_t* rgb, float* depth,
                                     uint8_t* inst, int32_t* face, int32_t* stats, void* stream)
{
    GDM_CHECK_ARG(verts && vcol && vnrm && faces && obj_face0 && slot_obj && RT && K && light && workspace && rgb && depth && inst && face &&
                      stats,
                  "gdm_render_frames_hip: NULL pointer");
    GDM_CHECK_ARG(n >= 1 && n <= 65535, "gdm_render_frames_hip: n=%d not in [1, 65535]", n);
    GDM_CHECK_ARG(S >= 1 && S <= GDM_RENDER_MAX_SLOTS, "gdm_render_frames_hip: S=%d not in [1, %d]", S, (int)GDM_RENDER_MAX_SLOTS);
    GDM_CHECK_ARG(O >= 1 && O <= GDM_RENDER_MAX_OBJECTS, "gdm_render_frames_hip: O=%d not in [1, %d]", O, (int)GDM_RENDER_MAX_OBJECTS);
    GDM_CHECK_ARG(Vt >= 1 && Ft >= 1, "gdm_render_frames_hip: Vt=%d Ft=%d must be positive", Vt, Ft);
    GDM_CHECK_ARG(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "gdm_render_frames_hip: H=%d W=%d not in [1, 16384]", H, W);
    GDM_CHECK_ARG(near >= 0.0, "gdm_render_frames_hip: near=%g must be >= 0", near);
    GDM_CHECK_ARG(ambient >= 0.0 && ambient <= 1.0, "gdm_render_frames_hip: ambient=%g not in [0, 1]", ambient);
    GDM_CHECK_ARG(k_per_instance == 0 || k_per_instance == 1, "gdm_render_frames_hip: k_per_instance=%d must be 0 or 1", k_per_instance);
    GDM_CHECK_ARG(verts_f64 == 0 || verts_f64 == 1, "gdm_render_frames_hip: verts_f64=%d must be 0 or 1", verts_f64);
    ObjTable tab = {};
    int Fmax = 0;
    GDM_CHECK_ARG(obj_face0[0] >= 0, "gdm_render_frames_hip: obj_face0[0]=%d must be >= 0", obj_face0[0]);
    for (int o = 0; o < O; ++o) {
        GDM_CHECK_ARG(obj_face0[o + 1] > obj_face0[o], "gdm_render_frames_hip: obj_face0 is not ascending at object %d (%d, then %d)", o,
                      obj_face0[o], obj_face0[o + 1]);
        Fmax = obj_face0[o + 1] - obj_face0[o] > Fmax ? obj_face0[o + 1] - obj_face0[o] : Fmax;
    }
    GDM_CHECK_ARG(obj_face0[O] <= Ft, "gdm_render_frames_hip: obj_face0[O]=%d exceeds Ft=%d", obj_face0[O], Ft);
    for (int o = 0; o <= O; ++o) tab.face0[o] = obj_face0[o];
    GDM_CHECK_ARG((long)n * S * Fmax <= (1L << 30), "gdm_render_frames_hip: n=%d S=%d too large for an object of %d faces (n S F <= 2^30)",
                  n, S, Fmax);
    const size_t need = gdm_render_frames_workspace_bytes(n, S, H, W);
    GDM_CHECK_ARG(workspace_bytes >= need, "gdm_render_frames_hip: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    GDM_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "gdm_render_frames_hip: workspace must be 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    u64* keys = (u64*)workspace;
    const long count = (long)n * S * H * W;
    const int fill_blocks = (int)(gdm_cdiv(count, kThreads) < 4096 ? gdm_cdiv(count, kThreads) : 4096);
    hipLaunchKernelGGL(clear_kernel, dim3(fill_blocks), dim3(kThreads), 0, s, keys, count, stats, n * S, H, W);
    int rc = gdm_launch_status("clear_kernel");
    if (rc) return rc;
    const dim3 vgrid(gdm_cdiv((long)n * S * Fmax, kThreads));
    const dim3 rgrid(gdm_cdiv((long)H * W, kThreads), n);
    if (verts_f64) {
        hipLaunchKernelGGL(vis_kernel<double>, vgrid, dim3(kThreads), 0, s, (const double*)verts, faces, slot_obj, tab, O, RT, K,
                           k_per_instance, n, S, Vt, Fmax, H, W, near, keys);
        rc = gdm_launch_status("vis_kernel");
        if (rc) return rc;
        hipLaunchKernelGGL(resolve_kernel<double>, rgrid, dim3(kThreads), 0, s, (const double*)verts, vcol, vnrm, faces, RT, K,
                           k_per_instance, light, ambient, near, S, Vt, Ft, H, W, keys, rgb, depth, inst, face, stats);
    } else {
        hipLaunchKernelGGL(vis_kernel<float>, vgrid, dim3(kThreads), 0, s, (const float*)verts, faces, slot_obj, tab, O, RT, K,
                           k_per_instance, n, S, Vt, Fmax, H, W, near, keys);
        rc = gdm_launch_status("vis_kernel");
        if (rc) return rc;
        hipLaunchKernelGGL(resolve_kernel<float>, rgrid, dim3(kThreads), 0, s, (const float*)verts, vcol, vnrm, faces, RT, K,
                           k_per_instance, light, ambient, near, S, Vt, Ft, H, W, keys, rgb, depth, inst, face, stats);
    }
    return gdm_launch_status("resolve_kernel");
}
