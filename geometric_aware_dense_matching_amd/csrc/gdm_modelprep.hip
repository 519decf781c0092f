// Object model preparation on the device, gfx950: from a triangle mesh to the [M,9] table every entry point of the package reads
// (xyz in mm, rgb 0..255, unit normal, rows in farthest-point order).  Three entries, each defined by a written rule in include/gdm.h
// that model_prep.py restates in numpy bit for bit:
//   gdm_surface_sample_hip   one thread per sample: four hash words -> a face by binary search in the integer cdf -> barycentric
//                            weights on 24-bit integers -> nine interpolated channels.  No atomics, any launch shape.
//   gdm_fps_wide_hip         farthest-point sampling with the candidates spread over the whole device: ONE LAUNCH PER PICK.  Every
//                            workgroup of launch i first reduces the packed partial maxima that launch i-1 left (so all of them know
//                            pick i-1), updates `dist` over its own slice and leaves its own partial in the other half of `partial`.
//                            Nothing waits for another workgroup inside a kernel: the order comes from the stream alone.
//   gdm_point_diameter_hip   the exact farthest pair: row tile i in registers, column tiles through LDS, one packed partial per
//                            workgroup, a second launch reduces them.  No atomics.
#include "gdm_common.h"
#include "gdm_texture.h"

namespace {

// lowbias32: the mixer of gdm_sample.hip and gdm_pose_robust.hip (include/gdm.h), repeated here bit for bit.
__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

constexpr int kSampleT = 256;

// The textured sampler's extra arguments (gdm_surface_sample_tex_hip): the face corners' (u, v), the texel buffer and the object's
// table row, validated by the entry.
struct SampleTex {
    const float* fuv;
    const uint32_t* tex;
    TexObj obj;
    int flip_v;
};
struct SampleNoTex {};

// TEX: the same draws, xyz and normal; the colour is the texture's level 0 at the interpolated (u, v) instead of the vertex colours'.
template <bool TEX>
__global__ __launch_bounds__(kSampleT) void surface_sample_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ faces, const float* __restrict__ vnrm, const float* __restrict__ vrgb,
    const int64_t* __restrict__ cdf, int F, int S, uint32_t seed, float* __restrict__ out,
    const std::conditional_t<TEX, SampleTex, SampleNoTex> st)
{
    const long s = (long)blockIdx.x * kSampleT + threadIdx.x;
    if (s >= S) return;
    const uint32_t base = mix32(mix32(seed ^ 0x9e3779b9u) ^ (uint32_t)s);
    const uint32_t h0 = mix32(base ^ 0x9e3779b9u), h1 = mix32(base ^ 0x3c6ef372u), h2 = mix32(base ^ 0xdaa66d2bu),
                   h3 = mix32(base ^ 0x78dde6e4u);                        // (j + 1) * 0x9e3779b9 mod 2^32, j = 0..3
    // the face: the first f with cdf[f] > target, target in [0, cdf[F-1])
    const unsigned long long total = (unsigned long long)cdf[F - 1];
    const long long target = (long long)__umul64hi(((unsigned long long)h0 << 32) | h1, total);
    int lo = 0, hi = F - 1;                                                // cdf[F-1] > target always
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    // barycentric weights on the 24-bit integers: u + v > 1 is decided exactly, and w0 = (1 - u) - v is exact and >= 0
    uint32_t ui = h2 >> 8, vi = h3 >> 8;
    if (ui + vi > (1u << 24)) { ui = (1u << 24) - ui; vi = (1u << 24) - vi; }
    const float u = __fmul_rn((float)ui, 5.9604644775390625e-08f), v = __fmul_rn((float)vi, 5.9604644775390625e-08f);
    const float w0 = __fsub_rn(__fsub_rn(1.f, u), v);
    const int32_t* fv = faces + (long)lo * 3;
    const long a = fv[0], b = fv[1], c = fv[2];
    float ch[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ch[k] = __fadd_rn(__fadd_rn(__fmul_rn(w0, verts[a * 3 + k]), __fmul_rn(u, verts[b * 3 + k])), __fmul_rn(v, verts[c * 3 + k]));
        ch[3 + k] = __fadd_rn(__fadd_rn(__fmul_rn(w0, vrgb[a * 3 + k]), __fmul_rn(u, vrgb[b * 3 + k])), __fmul_rn(v, vrgb[c * 3 + k]));
        ch[6 + k] = __fadd_rn(__fadd_rn(__fmul_rn(w0, vnrm[a * 3 + k]), __fmul_rn(u, vnrm[b * 3 + k])), __fmul_rn(v, vnrm[c * 3 + k]));
    }
    if constexpr (TEX) {
        const float* uv = st.fuv + (long)lo * 6;
        const float tu = __fadd_rn(__fadd_rn(__fmul_rn(w0, uv[0]), __fmul_rn(u, uv[2])), __fmul_rn(v, uv[4]));
        const float tv = __fadd_rn(__fadd_rn(__fmul_rn(w0, uv[1]), __fmul_rn(u, uv[3])), __fmul_rn(v, uv[5]));
        const uint32_t c = tex_fetch(st.tex, st.obj, 0, (double)tu, (double)tv, st.flip_v);
        ch[3] = (float)(c & 255u); ch[4] = (float)((c >> 8) & 255u); ch[5] = (float)((c >> 16) & 255u);
    } else {
#pragma unroll
        for (int k = 3; k < 6; ++k) ch[k] = fminf(fmaxf(floorf(__fadd_rn(ch[k], 0.5f)), 0.f), 255.f);
    }
    // sqrtf, not __fsqrt_rn: the compiler's header maps that one to the native square root (1 ulp), sqrtf is correctly rounded
    const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(ch[6], ch[6]), __fmul_rn(ch[7], ch[7])), __fmul_rn(ch[8], ch[8])));
    if (len > 0.f) {
#pragma unroll
        for (int k = 6; k < 9; ++k) ch[k] = __fdiv_rn(ch[k], len);
    }
    float* o = out + s * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = ch[k];
}

// ---- farthest-point sampling, one launch per pick ---------------------------------------------------------------------------
constexpr int kFpsT = 256;
constexpr int kFpsPerGroup = 1024;                                         // candidates per workgroup when the launcher chooses
constexpr int kFpsMaxGroups = 1024;

// max of a packed partial over the workgroup (kT threads); every thread returns it.  `sh` holds kT / 64 words.
template <int kT>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* sh)
{
#pragma unroll
    for (int mk = 1; mk < 64; mk <<= 1) {
        const uint32_t ohi = (uint32_t)__shfl_xor((int)(v >> 32), mk, 64), olo = (uint32_t)__shfl_xor((int)(v & 0xffffffffull), mk, 64);
        const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
        v = o > v ? o : v;
    }
    __syncthreads();                                                       // `sh` may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = sh[0];
#pragma unroll
    for (int w = 1; w < kT / 64; ++w) v = sh[w] > v ? sh[w] : v;
    return v;
}

// Launch i (1 .. m).  part_in: the `groups` partials of launch i-1 (unused for i == 1, where the last pick is index 0 and the old
// distance is 1e10 without a read); part_out: this launch's.  Launch m only stores the last pick (grid of one workgroup per cloud).
__global__ __launch_bounds__(kFpsT) void fps_wide_kernel(int n, int m, int groups, int i, const float* __restrict__ xyz,
                                                         float* __restrict__ dist, unsigned long long* __restrict__ partial,
                                                         int32_t* __restrict__ idx)
{
    __shared__ unsigned long long sh[kFpsT / 64];
    const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const float* p = xyz + (long)b * n * 3;
    float* t = dist + (long)b * n;
    unsigned long long* part = partial + (long)b * 2 * groups;
    int last = 0;
    if (i > 1) {
        const unsigned long long* in = part + (long)((i - 1) & 1) * groups;
        unsigned long long best = 0;
        for (int k = tid; k < groups; k += kFpsT) {
            const unsigned long long o = in[k];
            best = o > best ? o : best;
        }
        best = block_max_u64<kFpsT>(best, sh);
        last = (int)(0xffffffffu - (uint32_t)(best & 0xffffffffull));
    }
    if (g == 0 && tid == 0) idx[(long)b * m + (i - 1)] = last;
    if (i == m) return;
    const float lx = p[3 * (long)last], ly = p[3 * (long)last + 1], lz = p[3 * (long)last + 2];
    const long per = ((long)n + groups - 1) / groups;
    const long k0 = (long)g * per, k1 = k0 + per < n ? k0 + per : n;
    unsigned long long best = 0;                                           // an empty slice: below every real partial
    for (long k = k0 + tid; k < k1; k += kFpsT) {
        const float dx = __fsub_rn(p[3 * k], lx), dy = __fsub_rn(p[3 * k + 1], ly), dz = __fsub_rn(p[3 * k + 2], lz);
        float d2 = __fmul_rn(dx, dx);
        d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
        d2 = __fadd_rn(d2, __fmul_rn(dz, dz));
        const float v = fminf(i == 1 ? 1e10f : t[k], d2);
        t[k] = v;
        const unsigned long long o = ((unsigned long long)__float_as_uint(v) << 32) | (0xffffffffu - (uint32_t)k);
        best = o > best ? o : best;
    }
    best = block_max_u64<kFpsT>(best, sh);
    if (tid == 0) part[(long)(i & 1) * groups + g] = best;
}

// ---- the farthest pair ----------------------------------------------------------------------------------------------------
constexpr int kDiaT = 256;                                                 // points per tile = threads per workgroup
constexpr int kDiaChunks = 8;                                              // workgroups that share the column tiles of one row tile

__device__ __forceinline__ bool pair_before(uint32_t d, int i, int j, uint32_t od, int oi, int oj)
{
    return d > od || (d == od && (i < oi || (i == oi && j < oj)));
}

// Workgroup (ti, c): rows ti*256 .. +255, column tiles ti + c, ti + c + chunks, ...; partial[(ti * chunks + c) * 2 ..] =
// ((d2 bits << 32) | (0xffffffff - i), j), or (0, 0) when it saw no pair.
__global__ __launch_bounds__(kDiaT) void diameter_tiles_kernel(int V, int chunks, const float* __restrict__ xyz,
                                                               unsigned long long* __restrict__ partial)
{
    __shared__ float4 tile[kDiaT];
    __shared__ uint32_t sd[kDiaT / 64];
    __shared__ int si[kDiaT / 64], sj[kDiaT / 64];
    const int ti = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int nt = (V + kDiaT - 1) / kDiaT;
    const int i = ti * kDiaT + tid;
    const bool live = i < V;
    const float xi = live ? xyz[3 * (long)i] : 0.f, yi = live ? xyz[3 * (long)i + 1] : 0.f, zi = live ? xyz[3 * (long)i + 2] : 0.f;
    float bd = -1.f;
    int bj = 0x7fffffff;
    for (int tj = ti + c; tj < nt; tj += chunks) {
        const int j0 = tj * kDiaT, jl = j0 + tid;
        __syncthreads();
        tile[tid] = jl < V ? make_float4(xyz[3 * (long)jl], xyz[3 * (long)jl + 1], xyz[3 * (long)jl + 2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        const int cnt = V - j0 < kDiaT ? V - j0 : kDiaT;
        const int q0 = tj == ti ? tid + 1 : 0;                             // j > i inside the diagonal tile
        if (live)
            for (int q = q0; q < cnt; ++q) {
                const float4 pj = tile[q];
                const float dx = __fsub_rn(xi, pj.x), dy = __fsub_rn(yi, pj.y), dz = __fsub_rn(zi, pj.z);
                float d2 = __fmul_rn(dx, dx);
                d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
                d2 = __fadd_rn(d2, __fmul_rn(dz, dz));
                if (d2 > bd) {                                             // ascending j: the first maximum of row i
                    bd = d2;
                    bj = j0 + q;
                }
            }
    }
    // the workgroup's best: largest d2, then lowest i, then lowest j (d2 >= 0, so its bits order as an unsigned; -1 = no pair)
    const bool has = bd >= 0.f;
    uint32_t d = has ? __float_as_uint(bd) : 0u;
    int ri = has ? i : 0x7fffffff, rj = bj;
#pragma unroll
    for (int mk = 1; mk < 64; mk <<= 1) {
        const uint32_t od = (uint32_t)__shfl_xor((int)d, mk, 64);
        const int oi = __shfl_xor(ri, mk, 64), oj = __shfl_xor(rj, mk, 64);
        if (pair_before(od, oi, oj, d, ri, rj)) { d = od; ri = oi; rj = oj; }
    }
    if ((tid & 63) == 0) { sd[tid >> 6] = d; si[tid >> 6] = ri; sj[tid >> 6] = rj; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kDiaT / 64; ++w)
            if (pair_before(sd[w], si[w], sj[w], d, ri, rj)) { d = sd[w]; ri = si[w]; rj = sj[w]; }
        unsigned long long* o = partial + ((long)ti * chunks + c) * 2;
        const bool any = ri != 0x7fffffff;
        o[0] = any ? ((unsigned long long)d << 32) | (0xffffffffu - (uint32_t)ri) : 0ull;
        o[1] = any ? (unsigned long long)rj : 0ull;
    }
}

__global__ __launch_bounds__(kDiaT) void diameter_reduce_kernel(long count, const unsigned long long* __restrict__ partial,
                                                                int32_t* __restrict__ pair, float* __restrict__ d2)
{
    __shared__ unsigned long long sk[kDiaT], sj[kDiaT];
    const int tid = threadIdx.x;
    unsigned long long key = 0, j = 0;
    for (long k = tid; k < count; k += kDiaT) {
        const unsigned long long ok = partial[2 * k], oj = partial[2 * k + 1];
        if (ok > key || (ok == key && oj < j)) { key = ok; j = oj; }
    }
    sk[tid] = key;
    sj[tid] = j;
    __syncthreads();
    for (int st = kDiaT / 2; st > 0; st >>= 1) {
        if (tid < st) {
            const unsigned long long ok = sk[tid + st], oj = sj[tid + st];
            if (ok > sk[tid] || (ok == sk[tid] && oj < sj[tid])) { sk[tid] = ok; sj[tid] = oj; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        pair[0] = (int32_t)(0xffffffffu - (uint32_t)(sk[0] & 0xffffffffull));
        pair[1] = (int32_t)sj[0];
        d2[0] = __uint_as_float((uint32_t)(sk[0] >> 32));
    }
}

int dia_chunks(int V)
{
    const int nt = (V + kDiaT - 1) / kDiaT;
    return nt < kDiaChunks ? nt : kDiaChunks;
}

} // namespace

extern "C" int gdm_surface_sample_hip(const float* verts, const int32_t* faces, const float* vnrm, const float* vrgb, const int64_t* cdf,
                                      int V, int F, long S, uint32_t seed, float* out, void* stream)
{
    GDM_CHECK_ARG(verts && faces && vnrm && vrgb && cdf && out, "gdm_surface_sample_hip: NULL pointer");
    GDM_CHECK_ARG(V >= 1 && F >= 1, "gdm_surface_sample_hip: V=%d F=%d must both be at least 1", V, F);
    GDM_CHECK_ARG(S >= 1 && S < (1l << 31), "gdm_surface_sample_hip: S=%ld not in [1, 2^31)", S);
    hipLaunchKernelGGL(surface_sample_kernel<false>, dim3(gdm_cdiv(S, kSampleT)), dim3(kSampleT), 0, (hipStream_t)stream, verts, faces,
                       vnrm, vrgb, cdf, F, (int)S, seed, out, SampleNoTex{});
    return gdm_launch_status("surface_sample_kernel");
}

extern "C" int gdm_surface_sample_tex_hip(const float* verts, const int32_t* faces, const float* vnrm, const float* vrgb,
                                          const int64_t* cdf, const float* fuv, const void* tex, int64_t tex_off, int64_t tex_w,
                                          int64_t tex_h, int64_t tex_levels, long tex_texels, int flip_v, int V, int F, long S,
                                          uint32_t seed, float* out, void* stream)
{
    GDM_CHECK_ARG(verts && faces && vnrm && vrgb && cdf && fuv && tex && out, "gdm_surface_sample_tex_hip: NULL pointer");
    GDM_CHECK_ARG(V >= 1 && F >= 1, "gdm_surface_sample_tex_hip: V=%d F=%d must both be at least 1", V, F);
    GDM_CHECK_ARG(S >= 1 && S < (1l << 31), "gdm_surface_sample_tex_hip: S=%ld not in [1, 2^31)", S);
    GDM_CHECK_ARG(tex_texels >= 1 && tex_texels < (1l << 31), "gdm_surface_sample_tex_hip: tex_texels=%ld not in [1, 2^31)", tex_texels);
    GDM_CHECK_ARG(((uintptr_t)tex & 3) == 0, "gdm_surface_sample_tex_hip: tex must be 4-byte aligned");
    GDM_CHECK_ARG(flip_v == 0 || flip_v == 1, "gdm_surface_sample_tex_hip: flip_v=%d must be 0 or 1", flip_v);
    const dim3 grid(gdm_cdiv(S, kSampleT));
    if (tex_w == 0) {                                                      // no texture: the vertex colours, as gdm_surface_sample_hip
        hipLaunchKernelGGL(surface_sample_kernel<false>, grid, dim3(kSampleT), 0, (hipStream_t)stream, verts, faces, vnrm, vrgb, cdf, F,
                           (int)S, seed, out, SampleNoTex{});
        return gdm_launch_status("surface_sample_kernel");
    }
    SampleTex st = {fuv, (const uint32_t*)tex, {}, flip_v};
    GDM_CHECK_ARG(tex_row_valid(tex_off, tex_w, tex_h, tex_levels, tex_texels, st.obj),
                  "gdm_surface_sample_tex_hip: the row (offset %lld, %lld x %lld, %lld levels) does not lie inside %ld texels",
                  (long long)tex_off, (long long)tex_w, (long long)tex_h, (long long)tex_levels, tex_texels);
    hipLaunchKernelGGL(surface_sample_kernel<true>, grid, dim3(kSampleT), 0, (hipStream_t)stream, verts, faces, vnrm, vrgb, cdf, F, (int)S,
                       seed, out, st);
    return gdm_launch_status("surface_sample_kernel");
}

extern "C" int gdm_fps_wide_groups(int n)
{
    if (n < 1) return 0;
    const int g = gdm_cdiv(n, kFpsPerGroup);
    return g < kFpsMaxGroups ? g : kFpsMaxGroups;
}

extern "C" int gdm_fps_wide_hip(int B, int n, int m, int groups, const float* xyz, float* dist, void* partial, int32_t* idx, void* stream)
{
    GDM_CHECK_ARG(xyz && dist && partial && idx, "gdm_fps_wide_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && B <= 65535 && n >= 1 && m >= 1 && m <= n, "gdm_fps_wide_hip: bad shape B=%d n=%d m=%d", B, n, m);
    GDM_CHECK_ARG(groups >= 0 && groups <= kFpsMaxGroups, "gdm_fps_wide_hip: groups=%d not in [0, %d]", groups, kFpsMaxGroups);
    GDM_CHECK_ARG(((uintptr_t)partial & 7) == 0, "gdm_fps_wide_hip: partial must be 8-byte aligned");
    if (groups == 0) groups = gdm_fps_wide_groups(n);
    const hipStream_t s = (hipStream_t)stream;
    for (int i = 1; i <= m; ++i)
        hipLaunchKernelGGL(fps_wide_kernel, dim3(i == m ? 1 : groups, B), dim3(kFpsT), 0, s, n, m, groups, i, xyz, dist,
                           (unsigned long long*)partial, idx);
    return gdm_launch_status("fps_wide_kernel");
}

extern "C" size_t gdm_point_diameter_workspace_bytes(int V)
{
    if (V < 2 || V > (1 << 24)) return 0;
    return (size_t)((V + kDiaT - 1) / kDiaT) * dia_chunks(V) * 16;
}

extern "C" int gdm_point_diameter_hip(const float* xyz, int V, int64_t* workspace, size_t workspace_bytes, int32_t* pair, float* d2,
                                      void* stream)
{
    GDM_CHECK_ARG(xyz && workspace && pair && d2, "gdm_point_diameter_hip: NULL pointer");
    GDM_CHECK_ARG(V >= 2 && V <= (1 << 24), "gdm_point_diameter_hip: V=%d not in [2, 2^24]", V);
    const size_t need = gdm_point_diameter_workspace_bytes(V);
    GDM_CHECK_ARG(workspace_bytes >= need, "gdm_point_diameter_hip: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    GDM_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "gdm_point_diameter_hip: workspace must be 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const int nt = (V + kDiaT - 1) / kDiaT, chunks = dia_chunks(V);
    hipLaunchKernelGGL(diameter_tiles_kernel, dim3(nt, chunks), dim3(kDiaT), 0, s, V, chunks, xyz, (unsigned long long*)workspace);
    int rc = gdm_launch_status("diameter_tiles_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(diameter_reduce_kernel, dim3(1), dim3(kDiaT), 0, s, (long)nt * chunks, (const unsigned long long*)workspace, pair, d2);
    return gdm_launch_status("diameter_reduce_kernel");
}
