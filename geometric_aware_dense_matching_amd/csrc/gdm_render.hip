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
//                    (integer adds, minima and maxima are order-independent).  Its second instance, resolve_kernel<VT, true>
//                    (gdm_render_frames_tex_hip), colours the pixels whose winner's object has a valid row in the
//                    texture table from that object's pyramid by THE TEXTURE RULE (gdm_texture.h): the corner (u, v) interpolated
//                    like every attribute, once more at (px + 1, py) and (px, py + 1) for the level, then four dword loads and an
//                    integer blend.  The branch is compiled out of the first instance, which stays what it was.
// No allocation and no host read in the entry points: they capture in a hipGraph.
#include "gdm_common.h"
#include "gdm_raster.h"
#include "gdm_texture.h"

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

// What the textured resolve needs beyond the untextured one (gdm_render_frames_tex_hip); NoTex for the instance without the branch.
struct TexArgs {
    const float* fuv;                                                      // f32[Ft,3,2]: a (u, v) per face corner
    const uint32_t* tex;                                                   // every object's pyramid, tex_texels texels
    const int64_t* tab;                                                    // i64[O,4] = (offset, W0, H0, L): device data, validated per use
    const int32_t* slot_obj;
    long tex_texels;
    int O, flip_v;
};
struct NoTex {};

template <typename VT, bool TEX>
__global__ __launch_bounds__(kThreads) void resolve_kernel(const VT* __restrict__ verts, const uint8_t* __restrict__ vcol,
                                                           const float* __restrict__ vnrm, const int32_t* __restrict__ faces,
                                                           const double* __restrict__ RT, const double* __restrict__ Kmat,
                                                           int k_per_instance, const double* __restrict__ light, double ambient, double near,
                                                           int S, int Vt, int Ft, int H, int W, const u64* __restrict__ keys,
                                                           uint8_t* __restrict__ rgb, float* __restrict__ depth, uint8_t* __restrict__ inst,
                                                           int32_t* __restrict__ face, int32_t* __restrict__ stats,
                                                           const std::conditional_t<TEX, TexArgs, NoTex> ta)
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
                // the winner's object decides the branch: whole waves take one side wherever a wave's pixels show one object
                TexObj to = {};
                bool textured = false;
                if constexpr (TEX) {
                    const int o = ta.slot_obj[(long)b * S + win];
                    if (o >= 0 && o < ta.O) {
                        const int64_t* row = ta.tab + (long)o * 4;
                        textured = tex_row_valid(row[0], row[1], row[2], row[3], ta.tex_texels, to);
                    }
                }
                if (textured) {
                    if constexpr (TEX) {
                        const float* uv = ta.fuv + (long)f * 6;            // the corners follow the winding like the vertices
                        const int k1 = swapped ? 2 : 1, k2 = swapped ? 1 : 2;
                        const double u0 = (double)uv[0], v0 = (double)uv[1], u1 = (double)uv[k1 * 2], v1 = (double)uv[k1 * 2 + 1],
                                     u2 = (double)uv[k2 * 2], v2 = (double)uv[k2 * 2 + 1];
                        const double u = interp(q0, q1, q2, Q, u0, u1, u2), v = interp(q0, q1, q2, Q, v0, v1, v2);
                        // the same face at (px + 1, py) and (px, py + 1), covered or not: the edge functions are evaluated there
                        const long long X = (long long)px * 256, Y = (long long)py * 256;
                        double dU[2], dV[2];
                        bool fine = true;
#pragma unroll
                        for (int d = 0; d < 2; ++d) {
                            const long long Xn = X + (d == 0 ? 256 : 0), Yn = Y + (d == 0 ? 0 : 256);
                            const double p0 = (double)edge_fn(t.x1, t.y1, t.x2, t.y2, Xn, Yn) * t.iz0;
                            const double p1 = (double)edge_fn(t.x2, t.y2, t.x0, t.y0, Xn, Yn) * t.iz1;
                            const double p2 = (double)edge_fn(t.x0, t.y0, t.x1, t.y1, Xn, Yn) * t.iz2;
                            const double Qn = (p0 + p1) + p2;
                            fine = fine && Qn > 0.0;
                            dU[d] = interp(p0, p1, p2, Qn, u0, u1, u2) * (double)to.W0 - u * (double)to.W0;
                            dV[d] = interp(p0, p1, p2, Qn, v0, v1, v2) * (double)to.H0 - v * (double)to.H0;
                        }
                        const double ra = dU[0] * dU[0] + dV[0] * dV[0], rb = dU[1] * dU[1] + dV[1] * dV[1];
                        const int level = fine ? tex_level(ra >= rb ? ra : (rb > ra ? rb : ra + rb), to.L) : to.L - 1;        // the larger; NaN if either is
                        const uint32_t c = tex_fetch(ta.tex, to, level, u, v, ta.flip_v);
                        r = (int)fmin(255.0, floor((double)(c & 255u) * k + 0.5));
                        g = (int)fmin(255.0, floor((double)((c >> 8) & 255u) * k + 0.5));
                        bl = (int)fmin(255.0, floor((double)((c >> 16) & 255u) * k + 0.5));
                    }
                } else {
                    r = (int)fmin(255.0, floor(interp(q0, q1, q2, Q, (double)c0[0], (double)c1[0], (double)c2[0]) * k + 0.5));
                    g = (int)fmin(255.0, floor(interp(q0, q1, q2, Q, (double)c0[1], (double)c1[1], (double)c2[1]) * k + 0.5));
                    bl = (int)fmin(255.0, floor(interp(q0, q1, q2, Q, (double)c0[2], (double)c1[2], (double)c2[2]) * k + 0.5));
                }
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

namespace {

// Both entries: the checks, the clear and visibility passes, and the resolve pass with (ta != nullptr) or without the texture branch.
// `who` names the entry in a refusal.
int render_frames(const char* who, const void* verts, int verts_f64, const uint8_t* vcol, const float* vnrm, const int32_t* faces,
                  const int32_t* obj_face0, const int32_t* slot_obj, const double* RT, const double* K, int k_per_instance,
                  const double* light, double ambient, double near, int n, int S, int O, int Vt, int Ft, int H, int W, void* workspace,
                  size_t workspace_bytes, uint8_t* rgb, float* depth, uint8_t* inst, int32_t* face, int32_t* stats, const TexArgs* ta,
                  void* stream)
{
    GDM_CHECK_ARG(verts && vcol && vnrm && faces && obj_face0 && slot_obj && RT && K && light && workspace && rgb && depth && inst && face &&
                      stats,
                  "%s: NULL pointer", who);
    GDM_CHECK_ARG(n >= 1 && n <= 65535, "%s: n=%d not in [1, 65535]", who, n);
    GDM_CHECK_ARG(S >= 1 && S <= GDM_RENDER_MAX_SLOTS, "%s: S=%d not in [1, %d]", who, S, (int)GDM_RENDER_MAX_SLOTS);
    GDM_CHECK_ARG(O >= 1 && O <= GDM_RENDER_MAX_OBJECTS, "%s: O=%d not in [1, %d]", who, O, (int)GDM_RENDER_MAX_OBJECTS);
    GDM_CHECK_ARG(Vt >= 1 && Ft >= 1, "%s: Vt=%d Ft=%d must be positive", who, Vt, Ft);
    GDM_CHECK_ARG(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "%s: H=%d W=%d not in [1, 16384]", who, H, W);
    GDM_CHECK_ARG(near >= 0.0, "%s: near=%g must be >= 0", who, near);
    GDM_CHECK_ARG(ambient >= 0.0 && ambient <= 1.0, "%s: ambient=%g not in [0, 1]", who, ambient);
    GDM_CHECK_ARG(k_per_instance == 0 || k_per_instance == 1, "%s: k_per_instance=%d must be 0 or 1", who, k_per_instance);
    GDM_CHECK_ARG(verts_f64 == 0 || verts_f64 == 1, "%s: verts_f64=%d must be 0 or 1", who, verts_f64);
    if (ta) {
        GDM_CHECK_ARG(ta->fuv && ta->tex && ta->tab, "%s: NULL pointer", who);
        GDM_CHECK_ARG(ta->tex_texels >= 1 && ta->tex_texels < (1l << 31), "%s: tex_texels=%ld not in [1, 2^31)", who, ta->tex_texels);
        GDM_CHECK_ARG(((uintptr_t)ta->tex & 3) == 0, "%s: tex must be 4-byte aligned", who);
        GDM_CHECK_ARG(((uintptr_t)ta->tab & 7) == 0, "%s: tex_tab must be 8-byte aligned", who);
        GDM_CHECK_ARG(ta->flip_v == 0 || ta->flip_v == 1, "%s: flip_v=%d must be 0 or 1", who, ta->flip_v);
    }
    ObjTable tab = {};
    int Fmax = 0;
    GDM_CHECK_ARG(obj_face0[0] >= 0, "%s: obj_face0[0]=%d must be >= 0", who, obj_face0[0]);
    for (int o = 0; o < O; ++o) {
        GDM_CHECK_ARG(obj_face0[o + 1] > obj_face0[o], "%s: obj_face0 is not ascending at object %d (%d, then %d)", who, o, obj_face0[o],
                      obj_face0[o + 1]);
        Fmax = obj_face0[o + 1] - obj_face0[o] > Fmax ? obj_face0[o + 1] - obj_face0[o] : Fmax;
    }
    GDM_CHECK_ARG(obj_face0[O] <= Ft, "%s: obj_face0[O]=%d exceeds Ft=%d", who, obj_face0[O], Ft);
    for (int o = 0; o <= O; ++o) tab.face0[o] = obj_face0[o];
    GDM_CHECK_ARG((long)n * S * Fmax <= (1L << 30), "%s: n=%d S=%d too large for an object of %d faces (n S F <= 2^30)", who, n, S, Fmax);
    const size_t need = gdm_render_frames_workspace_bytes(n, S, H, W);
    GDM_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    GDM_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    const hipStream_t s = (hipStream_t)stream;
    u64* keys = (u64*)workspace;
    const long count = (long)n * S * H * W;
    const int fill_blocks = (int)(gdm_cdiv(count, kThreads) < 4096 ? gdm_cdiv(count, kThreads) : 4096);
    hipLaunchKernelGGL(clear_kernel, dim3(fill_blocks), dim3(kThreads), 0, s, keys, count, stats, n * S, H, W);
    int rc = gdm_launch_status("clear_kernel");
    if (rc) return rc;
    const dim3 vgrid(gdm_cdiv((long)n * S * Fmax, kThreads));
    const dim3 rgrid(gdm_cdiv((long)H * W, kThreads), n);
    gdm_dispatch_bool(verts_f64 != 0, [&](auto f64) {
        using VT = std::conditional_t<decltype(f64)::value, double, float>;
        hipLaunchKernelGGL((vis_kernel<VT>), vgrid, dim3(kThreads), 0, s, (const VT*)verts, faces, slot_obj, tab, O, RT, K, k_per_instance,
                           n, S, Vt, Fmax, H, W, near, keys);
        rc = gdm_launch_status("vis_kernel");
        if (rc) return;
        if (ta)
            hipLaunchKernelGGL((resolve_kernel<VT, true>), rgrid, dim3(kThreads), 0, s, (const VT*)verts, vcol, vnrm, faces, RT, K,
                               k_per_instance, light, ambient, near, S, Vt, Ft, H, W, keys, rgb, depth, inst, face, stats, *ta);
        else
            hipLaunchKernelGGL((resolve_kernel<VT, false>), rgrid, dim3(kThreads), 0, s, (const VT*)verts, vcol, vnrm, faces, RT, K,
                               k_per_instance, light, ambient, near, S, Vt, Ft, H, W, keys, rgb, depth, inst, face, stats, NoTex{});
        rc = gdm_launch_status("resolve_kernel");
    });
    return rc;
}

} // namespace

extern "C" int gdm_render_frames_hip(const void* verts, int verts_f64, const uint8_t* vcol, const float* vnrm, const int32_t* faces,
                                     const int32_t* obj_face0, const int32_t* slot_obj, const double* RT, const double* K,
                                     int k_per_instance, const double* light, double ambient, double near, int n, int S, int O, int Vt,
                                     int Ft, int H, int W, void* workspace, size_t workspace_bytes, uint8_t* rgb, float* depth,
                                     uint8_t* inst, int32_t* face, int32_t* stats, void* stream)
{
    return render_frames("gdm_render_frames_hip", verts, verts_f64, vcol, vnrm, faces, obj_face0, slot_obj, RT, K, k_per_instance, light,
                         ambient, near, n, S, O, Vt, Ft, H, W, workspace, workspace_bytes, rgb, depth, inst, face, stats, nullptr, stream);
}

extern "C" int gdm_render_frames_tex_hip(const void* verts, int verts_f64, const uint8_t* vcol, const float* vnrm, const int32_t* faces,
                                         const int32_t* obj_face0, const int32_t* slot_obj, const double* RT, const double* K,
                                         int k_per_instance, const double* light, double ambient, double near, int n, int S, int O, int Vt,
                                         int Ft, int H, int W, void* workspace, size_t workspace_bytes, uint8_t* rgb, float* depth,
                                         uint8_t* inst, int32_t* face, int32_t* stats, const float* fuv, const void* tex,
                                         const int64_t* tex_tab, long tex_texels, int flip_v, void* stream)
{
    const TexArgs ta = {fuv, (const uint32_t*)tex, tex_tab, slot_obj, tex_texels, O, flip_v};
    return render_frames("gdm_render_frames_tex_hip", verts, verts_f64, vcol, vnrm, faces, obj_face0, slot_obj, RT, K, k_per_instance,
                         light, ambient, near, n, S, O, Vt, Ft, H, W, workspace, workspace_bytes, rgb, depth, inst, face, stats, &ta, stream);
}
