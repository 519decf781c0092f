// Ground-truth correspondence targets on the device, gfx950: the reference loader's get_pose_gt_info
// (datasets/lm/linemod_pbr.py:602-655) for a whole batch, hidden-point removal included.
//   hpr_flip_kernel         one workgroup per crop: camera centre, the spherical flip (utils/compute_visibility.py:26-37 sphericalFlip)
//                           in the reference's fp32 / fp64 operation order, and the fp64 sum of the flipped points
//   hpr_order_kernel        the constraint order of the LP test below: a hashed permutation of 0..M-1 shared by every crop
//   hpr_hull_kernel         one wave per (crop, vertex): is f_i a vertex of conv({f} U {0})?  Exact extreme-point test in fp64
//                           as a 2-D LP feasibility problem (Seidel's incremental algorithm, one constraint per lane)
//   hpr_finish_kernel       one workgroup per crop: is the origin a vertex, then the reference's vertices[:-1] (:128-134)
//   targets_compact_kernel  one workgroup per crop: the visible vertices in index order, posed in fp32 (linemod_pbr.py:633-636)
//   targets_nn_kernel       one thread per (crop, point): the nearest posed visible vertex, d^2 in fp64, and the 1 cm test (:638-651)
//   targets_finish_kernel   the outputs, with the reference's two early returns (:626-630, :644-646)
// No allocation and no host synchronisation: the whole chain captures in a hipGraph.
#include "gdm_common.h"

namespace {

constexpr double HPR_PARAM = 0x1.5a5d2ab3e544ap+10;      // np.power(10.0, math.pi) = 1385.4557313670107 (compute_visibility.py:131)
constexpr double LP_BOX = 1e6;                            // |a|, |b| <= LP_BOX: separating directions within 1e-6 rad of f_i's
                                                          // normal plane are not searched (include/gdm.h)
constexpr int NN_TILE = 1024;

// One LP constraint of the test of base point o (a vertex f_i, or the origin): g = f_j - o in the frame (h, e1, e2);
// d = h + a e1 + b e2 separates o iff w + a u + b v < 0 for every constraint.  Skipped constraints come back as 0 <= 0.
__device__ __forceinline__ void lp_cons(const double* __restrict__ F, int j, int self, double ox, double oy, double oz, const double* h,
                                        const double* e1, const double* e2, double& w, double& u, double& v)
{
    const double gx = F[3 * (long)j] - ox, gy = F[3 * (long)j + 1] - oy, gz = F[3 * (long)j + 2] - oz;
    if (j == self || (j > self && self >= 0 && gx == 0.0 && gy == 0.0 && gz == 0.0)) { w = 0.0; u = 0.0; v = 0.0; return; }
    w = (h[0] * gx + h[1] * gy) + h[2] * gz;
    u = (e1[0] * gx + e1[1] * gy) + e1[2] * gz;
    v = (e2[0] * gx + e2[1] * gy) + e2[2] * gz;
}

// An orthonormal frame (h, e1, e2) around the unit axis h.
__device__ __forceinline__ void lp_frame(const double* h, double* e1, double* e2)
{
    const double ax = fabs(h[0]), ay = fabs(h[1]), az = fabs(h[2]);
    const int k = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);          // the coordinate axis least aligned with h
    double c[3];
    if (k == 0)      { c[0] = 0.0;   c[1] = h[2];  c[2] = -h[1]; }         // h x x_k
    else if (k == 1) { c[0] = -h[2]; c[1] = 0.0;   c[2] = h[0]; }
    else             { c[0] = h[1];  c[1] = -h[0]; c[2] = 0.0; }
    const double cn = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    e1[0] = c[0] / cn; e1[1] = c[1] / cn; e1[2] = c[2] / cn;
    e2[0] = h[1] * e1[2] - h[2] * e1[1];
    e2[1] = h[2] * e1[0] - h[0] * e1[2];
    e2[2] = h[0] * e1[1] - h[1] * e1[0];
}

__device__ __forceinline__ double wave_max_f64(double x)
{
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

__device__ __forceinline__ double wave_min_f64(double x)
{
    for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o, 64));
    return x;
}

// Whole-wave test: does a direction d with d . (f_j - o) < 0 for all j (minus the skipped ones) exist, given that every such d has
// d . h > 0?  Returns 1 (o is a vertex), 0 (it is not).  F = the crop's f64[M][3]; perm = the constraint order.  Called by all 64 lanes.
__device__ int lp_vertex(const double* __restrict__ F, const int32_t* __restrict__ perm, int M, int self, double ox, double oy,
                         double oz, const double* h)
{
    const int lane = threadIdx.x & 63;
    double e1[3], e2[3];
    lp_frame(h, e1, e2);
    // Pass 1, in index order: an exact duplicate of lower index rules the point out; (a, b) = (0, 0) feasible proves it a vertex.
    bool dup = false, all_neg = true;
    for (int j0 = 0; j0 < M; j0 += 64) {
        const int j = j0 + lane;
        if (j < M && j != self) {
            const double gx = F[3 * (long)j] - ox, gy = F[3 * (long)j + 1] - oy, gz = F[3 * (long)j + 2] - oz;
            if (gx == 0.0 && gy == 0.0 && gz == 0.0) {
                if (j < self) dup = true;
            } else if (!(((h[0] * gx + h[1] * gy) + h[2] * gz) < 0.0)) {
                all_neg = false;
            }
        }
    }
    if (__any(dup)) return 0;
    if (__all(all_neg)) return 1;
    // Pass 2: Seidel's incremental 2-D LP, minimise a over the box |a|, |b| <= LP_BOX and the constraints in `perm` order.  The
    // optimum x moves only when a constraint rejects it, and then onto that constraint's line (a 1-D LP over the earlier ones).
    double xa = -LP_BOX, xb = -LP_BOX;
    for (int k0 = 0; k0 < M; k0 += 64) {
        const int k = k0 + lane;
        double w = 0.0, u = 0.0, v = 0.0;
        if (k < M) lp_cons(F, perm[k], self, ox, oy, oz, h, e1, e2, w, u, v);
        int start = 0;
        for (;;) {
            const bool viol = lane >= start && (w + xa * u) + xb * v > 0.0;
            const unsigned long long bal = __ballot(viol);
            if (bal == 0ull) break;
            const int kl = __ffsll((long long)bal) - 1;
            const double uk = __shfl(u, kl, 64), vk = __shfl(v, kl, 64), wk = __shfl(w, kl, 64);
            const double nn2 = uk * uk + vk * vk;
            if (nn2 == 0.0) return 0;                                     // 0 a + 0 b + wk <= 0 with wk > 0
            const double pa = -wk * uk / nn2, pb = -wk * vk / nn2;        // a point of the line, and its direction
            const double da = -vk, db = uk;
            double tlo = -INFINITY, thi = INFINITY;
            bool bad = false;
            // the box
            if (da > 0.0) { thi = fmin(thi, (LP_BOX - pa) / da); tlo = fmax(tlo, (-LP_BOX - pa) / da); }
            else if (da < 0.0) { thi = fmin(thi, (-LP_BOX - pa) / da); tlo = fmax(tlo, (LP_BOX - pa) / da); }
            else if (fabs(pa) > LP_BOX) bad = true;
            if (db > 0.0) { thi = fmin(thi, (LP_BOX - pb) / db); tlo = fmax(tlo, (-LP_BOX - pb) / db); }
            else if (db < 0.0) { thi = fmin(thi, (-LP_BOX - pb) / db); tlo = fmax(tlo, (LP_BOX - pb) / db); }
            else if (fabs(pb) > LP_BOX) bad = true;
            // the constraints before it in the order: alpha t <= beta
            const int K = k0 + kl;
            for (int q0 = 0; q0 < K; q0 += 64) {
                const int q = q0 + lane;
                if (q < K) {
                    double wq, uq, vq;
                    lp_cons(F, perm[q], self, ox, oy, oz, h, e1, e2, wq, uq, vq);
                    const double al = uq * da + vq * db;
                    const double be = -wq - (uq * pa + vq * pb);
                    if (al > 0.0) thi = fmin(thi, be / al);
                    else if (al < 0.0) tlo = fmax(tlo, be / al);
                    else if (be < 0.0) bad = true;
                }
            }
            tlo = wave_max_f64(tlo);
            thi = wave_min_f64(thi);
            if (__any(bad) || tlo > thi) return 0;
            const double t = da < 0.0 ? thi : tlo;
            xa = pa + t * da;
            xb = pb + t * db;
            start = kl + 1;
        }
    }
    return 1;
}

// f f64[B,M,3], csum f64[B,3] = sum of f (fixed order).
__global__ __launch_bounds__(1024) void hpr_flip_kernel(const float* __restrict__ model, long model_bstride, const float* __restrict__ RT,
                                                        const float* __restrict__ cam_center, int M, double* __restrict__ F,
                                                        double* __restrict__ csum)
{
    __shared__ float s_max[16];
    __shared__ double s_sum[16][3];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* r = RT + (long)b * 12;
    float c[3];
    for (int k = 0; k < 3; ++k) {
        if (cam_center) c[k] = cam_center[(long)b * 3 + k];
        else            c[k] = (float)(-((((double)r[k] * (double)r[3]) + (double)r[4 + k] * (double)r[7]) + (double)r[8 + k] * (double)r[11]));
    }
    const float* mp = model + (long)b * model_bstride;
    float mx = 0.f;
    for (int j = threadIdx.x; j < M; j += 1024) {                      // normPoints, fp32: sqrt((x^2 + y^2) + z^2)
        const float px = mp[3 * (long)j] - c[0], py = mp[3 * (long)j + 1] - c[1], pz = mp[3 * (long)j + 2] - c[2];
        mx = fmaxf(mx, sqrtf((px * px + py * py) + pz * pz));
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) s_max[wave] = mx;
    __syncthreads();
    mx = s_max[0];
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, s_max[w]);
    const double rad = (double)mx * HPR_PARAM;                         // R = max(normPoints) * 10^pi, fp64
    double sx = 0.0, sy = 0.0, sz = 0.0;
    double* Fb = F + (long)b * M * 3;
    for (int j = threadIdx.x; j < M; j += 1024) {                      // f = 2 (R - n) p / n + p, fp64
        const float px = mp[3 * (long)j] - c[0], py = mp[3 * (long)j + 1] - c[1], pz = mp[3 * (long)j + 2] - c[2];
        const double n = (double)sqrtf((px * px + py * py) + pz * pz);
        const double s = rad - n;
        const double fx = (2.0 * (s * (double)px)) / n + (double)px;
        const double fy = (2.0 * (s * (double)py)) / n + (double)py;
        const double fz = (2.0 * (s * (double)pz)) / n + (double)pz;
        Fb[3 * (long)j] = fx; Fb[3 * (long)j + 1] = fy; Fb[3 * (long)j + 2] = fz;
        sx += fx; sy += fy; sz += fz;
    }
    for (int o = 32; o > 0; o >>= 1) {
        sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); sz += __shfl_xor(sz, o, 64);
    }
    if (lane == 0) { s_sum[wave][0] = sx; s_sum[wave][1] = sy; s_sum[wave][2] = sz; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += s_sum[w][threadIdx.x];
        csum[(long)b * 3 + threadIdx.x] = t;
    }
}

// perm i32[M]: a bijection of [0, M) -- an invertible mix of m-bit integers (2^m >= M), cycle-walked into range.
__global__ __launch_bounds__(256) void hpr_order_kernel(int M, int32_t* __restrict__ perm)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= M) return;
    int m = 1;
    while ((1u << m) < (unsigned)M) ++m;
    const uint32_t mask = (m >= 32) ? 0xffffffffu : ((1u << m) - 1u);
    const int s = m > 2 ? m / 2 : 1;
    uint32_t x = (uint32_t)k;
    do {
        x = (x * 0x7feb352du + 0x9e3779b9u) & mask;
        x ^= x >> s;
        x = (x * 0x846ca68bu) & mask;
        x ^= x >> s;
    } while (x >= (uint32_t)M);
    perm[k] = (int32_t)x;
}

// visible u8[B,M]: 1 where f_i is a vertex of conv({f} U {0}) (before the vertices[:-1] rule).  One wave per vertex.
__global__ __launch_bounds__(256) void hpr_hull_kernel(const double* __restrict__ F, const int32_t* __restrict__ perm, int M,
                                                       uint8_t* __restrict__ visible)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= M) return;                                                // wave-uniform; no barrier below
    const double* Fb = F + (long)b * M * 3;
    const double fx = Fb[3 * (long)i], fy = Fb[3 * (long)i + 1], fz = Fb[3 * (long)i + 2];
    const double fn = sqrt((fx * fx + fy * fy) + fz * fz);
    int vis = 0;
    if (fn > 0.0) {                                                    // f_i = 0 is the origin itself: never a vertex of its own
        const double h[3] = {fx / fn, fy / fn, fz / fn};
        vis = lp_vertex(Fb, perm, M, i, fx, fy, fz, h);
    }
    if ((threadIdx.x & 63) == 0) visible[(long)b * M + i] = (uint8_t)vis;
}

// The origin's own test (d . f_j < 0 for all j, d . csum < 0 for any such d), then vertices[:-1]: when the origin is not a
// vertex, the highest-index visible model vertex is dropped.
__global__ __launch_bounds__(256) void hpr_finish_kernel(const double* __restrict__ F, const double* __restrict__ csum,
                                                         const int32_t* __restrict__ perm, int M, uint8_t* __restrict__ visible)
{
    __shared__ int s_origin;
    __shared__ int s_last[4];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {
        const double cx = csum[(long)b * 3], cy = csum[(long)b * 3 + 1], cz = csum[(long)b * 3 + 2];
        const double cn = sqrt((cx * cx + cy * cy) + cz * cz);
        int ov = 0;
        if (cn > 0.0) {
            const double h[3] = {-cx / cn, -cy / cn, -cz / cn};
            ov = lp_vertex(F + (long)b * M * 3, perm, M, -1, 0.0, 0.0, 0.0, h);
        }
        if (lane == 0) s_origin = ov;
    }
    int last = -1;
    for (int j = threadIdx.x; j < M; j += 256)
        if (visible[(long)b * M + j]) last = j;
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
    if (lane == 0) s_last[wave] = last;
    __syncthreads();
    if (threadIdx.x == 0 && !s_origin) {
        last = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
        if (last >= 0) visible[(long)b * M + last] = 0;
    }
}

// vxyz f32[B][3][M]: the visible vertices in index order, posed as ((r0 x + r1 y) + r2 z) + t; vidx i32[B][M] their model index;
// nvis i32[B]; cnt i32[B][2] (labelled points, fitted points) zeroed for targets_nn_kernel.
__global__ __launch_bounds__(1024) void targets_compact_kernel(const float* __restrict__ model, long model_bstride,
                                                               const float* __restrict__ RT, const uint8_t* __restrict__ visible, int M,
                                                               float* __restrict__ vxyz, int32_t* __restrict__ vidx,
                                                               int32_t* __restrict__ nvis, int32_t* __restrict__ cnt)
{
    __shared__ int wtot[16];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* r = RT + (long)b * 12;
    const float* mp = model + (long)b * model_bstride;
    float* V = vxyz + (long)b * 3 * M;
    int run = 0;
    for (int c0 = 0; c0 < M; c0 += 1024) {
        const int j = c0 + threadIdx.x;
        const bool sel = j < M && visible[(long)b * M + j];
        const unsigned long long bal = __ballot(sel);
        const int below = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        int off = run;
        for (int w = 0; w < wave; ++w) off += wtot[w];
        if (sel) {
            const float x = mp[3 * (long)j], y = mp[3 * (long)j + 1], z = mp[3 * (long)j + 2];
            const int k = off + below;
            V[k] = ((r[0] * x + r[1] * y) + r[2] * z) + r[3];
            V[M + k] = ((r[4] * x + r[5] * y) + r[6] * z) + r[7];
            V[2 * M + k] = ((r[8] * x + r[9] * y) + r[10] * z) + r[11];
            vidx[(long)b * M + k] = j;
        }
        for (int w = 0; w < 16; ++w) run += wtot[w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        nvis[b] = run;
        cnt[2 * b] = 0;
        cnt[2 * b + 1] = 0;
    }
}

// tmatch i32[B,N]: for a labelled point the model index of its nearest visible vertex, or M beyond the threshold; M otherwise.
// Nearest = smallest fp64 ((dx^2 + dy^2) + dz^2) from the fp32 coordinates, ties to the lowest model index.
__global__ __launch_bounds__(256) void targets_nn_kernel(const float* __restrict__ cld, long cld_bstride, int pt_stride, int ch_stride,
                                                         const uint8_t* __restrict__ labels, const float* __restrict__ vxyz,
                                                         const int32_t* __restrict__ vidx, const int32_t* __restrict__ nvis, int N, int M,
                                                         double thresh, int32_t* __restrict__ tmatch, int32_t* __restrict__ cnt)
{
    __shared__ float s_v[3][NN_TILE];
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool lab = i < N && labels[(long)b * N + i] > 0;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (lab) {
        const float* sp = cld + (long)b * cld_bstride + (long)i * pt_stride;
        px = (double)sp[0]; py = (double)sp[ch_stride]; pz = (double)sp[2 * ch_stride];
    }
    const int nv = nvis[b];
    const float* V = vxyz + (long)b * 3 * M;
    double best = INFINITY;
    int bk = -1;
    for (int t0 = 0; t0 < nv; t0 += NN_TILE) {
        const int tn = min(NN_TILE, nv - t0);
        __syncthreads();
        for (int k = threadIdx.x; k < tn; k += 256) {
            s_v[0][k] = V[t0 + k];
            s_v[1][k] = V[M + t0 + k];
            s_v[2][k] = V[2 * M + t0 + k];
        }
        __syncthreads();
        if (lab) {
            for (int k = 0; k < tn; ++k) {
                const double dx = px - (double)s_v[0][k], dy = py - (double)s_v[1][k], dz = pz - (double)s_v[2][k];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < best) { best = d2; bk = t0 + k; }
            }
        }
    }
    const bool fit = lab && bk >= 0 && !(sqrt(best) > thresh);
    if (i < N) tmatch[(long)b * N + i] = fit ? vidx[(long)b * M + bk] : M;
    const int nl = __popcll(__ballot(lab)), nf = __popcll(__ballot(fit));
    if ((threadIdx.x & 63) == 0 && nl > 0) {
        atomicAdd(&cnt[2 * b], nl);
        if (nf > 0) atomicAdd(&cnt[2 * b + 1], nf);
    }
}

// labels and labels_out may alias (each thread reads its element before it writes it): neither is __restrict__.
__global__ __launch_bounds__(256) void targets_finish_kernel(const uint8_t* labels, const uint8_t* __restrict__ visible,
                                                             const int32_t* __restrict__ tmatch, const int32_t* __restrict__ cnt, int N,
                                                             int M, uint8_t* labels_out, int32_t* __restrict__ match_idx,
                                                             uint8_t* __restrict__ visible_flag, uint8_t* __restrict__ valid)
{
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int nl = cnt[2 * b], nf = cnt[2 * b + 1];
    const bool ok = nl > 0 && nf > 0;                                  // :626-630 no labelled point; :644-646 none within the threshold
    if (t < N) {
        const uint8_t l = labels[(long)b * N + t];
        const int m = ok ? tmatch[(long)b * N + t] : M;
        labels_out[(long)b * N + t] = (ok && l > 0 && m == M) ? (uint8_t)0 : l;
        match_idx[(long)b * N + t] = l > 0 ? m : M;
    }
    if (t < M) visible_flag[(long)b * M + t] = nl > 0 ? visible[(long)b * M + t] : (uint8_t)0;
    if (t == 0) valid[b] = ok ? 1 : 0;
}

struct TargetsWs {
    double* csum;
    int32_t* perm;
    size_t hpr_bytes;
    float* vxyz;
    int32_t* vidx;
    int32_t* nvis;
    int32_t* cnt;
    int32_t* tmatch;
    size_t bytes;
};

size_t ws_align(size_t x) { return (x + 255) & ~(size_t)255; }

TargetsWs targets_ws(void* base, int B, int N, int M)
{
    TargetsWs w;
    char* p = (char*)base;
    size_t o = 0;
    w.csum = (double*)(p + o); o += ws_align((size_t)B * 3 * sizeof(double));
    w.perm = (int32_t*)(p + o); o += ws_align((size_t)M * sizeof(int32_t));
    w.hpr_bytes = o;
    w.vxyz = (float*)(p + o);  o += ws_align((size_t)B * 3 * M * sizeof(float));
    w.vidx = (int32_t*)(p + o); o += ws_align((size_t)B * M * sizeof(int32_t));
    w.nvis = (int32_t*)(p + o); o += ws_align((size_t)B * sizeof(int32_t));
    w.cnt = (int32_t*)(p + o);  o += ws_align((size_t)B * 2 * sizeof(int32_t));
    w.tmatch = (int32_t*)(p + o); o += ws_align((size_t)B * N * sizeof(int32_t));
    w.bytes = o;
    return w;
}

} // namespace

extern "C" size_t gdm_targets_workspace_bytes(int B, int N, int M)
{
    if (B < 1 || N < 1 || M < GDM_TARGETS_MIN_M || B > 65535) return 0;
    return targets_ws(nullptr, B, N, M).bytes;
}

extern "C" int gdm_hpr_visible_hip(const float* model_xyz, long model_bstride, const float* RT, const float* cam_center, int B, int M,
                                   void* workspace, size_t workspace_bytes, double* flipped, uint8_t* visible, void* stream)
{
    GDM_CHECK_ARG(model_xyz && RT && workspace && flipped && visible, "gdm_hpr_visible_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && B <= 65535, "gdm_hpr_visible_hip: B=%d not in [1, 65535]", B);
    GDM_CHECK_ARG(M >= GDM_TARGETS_MIN_M, "gdm_hpr_visible_hip: M=%d < %d", M, GDM_TARGETS_MIN_M);
    GDM_CHECK_ARG(model_bstride == 0 || model_bstride >= 3L * M, "gdm_hpr_visible_hip: model_bstride=%ld (0 or >= 3 M)", model_bstride);
    const TargetsWs w = targets_ws(workspace, B, 1, M);
    GDM_CHECK_ARG(workspace_bytes >= w.hpr_bytes, "gdm_hpr_visible_hip: workspace of %zu bytes, %zu needed", workspace_bytes, w.hpr_bytes);
    GDM_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "gdm_hpr_visible_hip: workspace must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(hpr_flip_kernel, dim3(B), dim3(1024), 0, s, model_xyz, model_bstride, RT, cam_center, M, flipped, w.csum);
    int rc = gdm_launch_status("hpr_flip_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(hpr_order_kernel, dim3(gdm_cdiv(M, 256)), dim3(256), 0, s, M, w.perm);
    if ((rc = gdm_launch_status("hpr_order_kernel"))) return rc;
    hipLaunchKernelGGL(hpr_hull_kernel, dim3(gdm_cdiv(M, 4), B), dim3(256), 0, s, flipped, w.perm, M, visible);
    if ((rc = gdm_launch_status("hpr_hull_kernel"))) return rc;
    hipLaunchKernelGGL(hpr_finish_kernel, dim3(B), dim3(256), 0, s, flipped, w.csum, w.perm, M, visible);
    return gdm_launch_status("hpr_finish_kernel");
}

extern "C" int gdm_pose_targets_hip(const float* cld, long cld_bstride, int pt_stride, int ch_stride, const uint8_t* labels,
                                    const float* RT, const float* model_xyz, long model_bstride, const uint8_t* visible, int B, int N,
                                    int M, double dist_thresh, void* workspace, size_t workspace_bytes, uint8_t* labels_out,
                                    int32_t* match_idx, uint8_t* visible_flag, uint8_t* valid, void* stream)
{
    GDM_CHECK_ARG(cld && labels && RT && model_xyz && visible && workspace && labels_out && match_idx && visible_flag && valid,
                  "gdm_pose_targets_hip: NULL pointer");
    GDM_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1, "gdm_pose_targets_hip: bad shape B=%d N=%d", B, N);
    GDM_CHECK_ARG(M >= GDM_TARGETS_MIN_M, "gdm_pose_targets_hip: M=%d < %d", M, GDM_TARGETS_MIN_M);
    GDM_CHECK_ARG(pt_stride >= 1 && ch_stride >= 1 && cld_bstride >= 0, "gdm_pose_targets_hip: bad cld strides");
    GDM_CHECK_ARG(model_bstride == 0 || model_bstride >= 3L * M, "gdm_pose_targets_hip: model_bstride=%ld (0 or >= 3 M)", model_bstride);
    GDM_CHECK_ARG(dist_thresh > 0.0, "gdm_pose_targets_hip: dist_thresh=%g must be > 0", dist_thresh);
    const TargetsWs w = targets_ws(workspace, B, N, M);
    GDM_CHECK_ARG(workspace_bytes >= w.bytes, "gdm_pose_targets_hip: workspace of %zu bytes, %zu needed", workspace_bytes, w.bytes);
    GDM_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "gdm_pose_targets_hip: workspace must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(targets_compact_kernel, dim3(B), dim3(1024), 0, s, model_xyz, model_bstride, RT, visible, M, w.vxyz, w.vidx,
                       w.nvis, w.cnt);
    int rc = gdm_launch_status("targets_compact_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(targets_nn_kernel, dim3(gdm_cdiv(N, 256), B), dim3(256), 0, s, cld, cld_bstride, pt_stride, ch_stride, labels,
                       w.vxyz, w.vidx, w.nvis, N, M, dist_thresh, w.tmatch, w.cnt);
    if ((rc = gdm_launch_status("targets_nn_kernel"))) return rc;
    hipLaunchKernelGGL(targets_finish_kernel, dim3(gdm_cdiv(N > M ? N : M, 256), B), dim3(256), 0, s, labels, visible, w.tmatch, w.cnt,
                       N, M, labels_out, match_idx, visible_flag, valid);
    return gdm_launch_status("targets_finish_kernel");
}
