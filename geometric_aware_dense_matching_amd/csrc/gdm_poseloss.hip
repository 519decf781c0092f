// The differentiable pose-fit loss (include/gdm.h THE POSE LOSS RULE), gfx950: the ADD-style error of the weighted
// Kabsch fit of soft targets, forward and backward, so that training sees the metric the evaluator reports.
//
// Forward = the statistics launch of the weighted fit (gdm_kabsch_stats_w_hip itself: its usable points, its skip rule, its order of
// sums) and one workgroup of 256 threads per crop: lane 0 fits (the shared fragment gdm_kabsch_fit.inc, so RT is solve_poses_weighted's
// bit for bit) and judges the conditioning, the block sums the K x S distances in the fixed order of block_sum, lane 0 runs the adjoint
// of the fit (gdm_pose_adjoint.h: one 3x3 solve, no SVD derivative) and leaves a 32-double record per crop.
// Backward = one launch that reads the record and streams the points once (28 B read, 16 B written per point); no gradient of a point
// is a sum over other points, so there are no atomics and the bits do not depend on how often or how (eager, hipGraph) it runs.
// No library solver, no host read, a fixed launch count: the whole step captures in a hipGraph.
#include "gdm_pose_fit.h"
#include "gdm_pose_adjoint.h"

namespace {

// The record of one crop, doubles: what the backward needs, so that it does not refit.
enum { REC_CA = 0, REC_CB = 3, REC_W = 6, REC_GAMMA = 7, REC_RTG = 16, REC_G = 19, REC_STATE = 22, REC_R = 23 };
static_assert(REC_R + 9 == GDM_POSE_LOSS_REC, "the record is GDM_POSE_LOSS_REC doubles");

// The record buffer: the 16 statistics of every crop, the records, the usable-point counts.
struct RecordViews { double* stats; double* rec; int32_t* count; };
static inline RecordViews record_views(void* record, int B)
{
    double* base = (double*)record;
    return {base, base + (size_t)B * 16, (int32_t*)(base + (size_t)B * (16 + GDM_POSE_LOSS_REC))};
}

// e = (R X + t) - (Rg (Rs X + ts) + tg) in fp64, every sum in the written order.  pose = R (9, row-major) then t (3); gt and sym are
// [R | t] f32[3,4] rows; sym == NULL is the identity.
__device__ __forceinline__ void pose_error(const double* pose, const double* gt, const float* sym, double x, double y, double z, double* e)
{
    double qx = x, qy = y, qz = z;
    if (sym) {
        qx = (((double)sym[0] * x + (double)sym[1] * y) + (double)sym[2] * z) + (double)sym[3];
        qy = (((double)sym[4] * x + (double)sym[5] * y) + (double)sym[6] * z) + (double)sym[7];
        qz = (((double)sym[8] * x + (double)sym[9] * y) + (double)sym[10] * z) + (double)sym[11];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double p = ((pose[3 * i] * x + pose[3 * i + 1] * y) + pose[3 * i + 2] * z) + pose[9 + i];
        const double m = ((gt[4 * i] * qx + gt[4 * i + 1] * qy) + gt[4 * i + 2] * qz) + gt[4 * i + 3];
        e[i] = p - m;
    }
}

__global__ __launch_bounds__(256) void pose_loss_fwd_kernel(const double* __restrict__ stats, const int32_t* __restrict__ count,
                                                            const float* __restrict__ RT_gt, const float* __restrict__ model_pts,
                                                            const float* __restrict__ sym, int K, int S, int min_points, double cond_min,
                                                            double* __restrict__ rec, double* __restrict__ loss, float* __restrict__ RT,
                                                            uint8_t* __restrict__ state, int32_t* __restrict__ sym_idx)
{
    __shared__ double red1[4][1];
    __shared__ double red12[4][12];
    __shared__ double fit[25];                                         // R (9), t (3), the ground truth (12), the state
    const int b = blockIdx.x;
    double* r = rec + (long)b * GDM_POSE_LOSS_REC;
    double Rd[3][3], cAd[3], lam[3], V[3][3];                           // lane 0 keeps them for the adjoint
    if (threadIdx.x == 0) {
        const double* st = stats + (long)b * 16;
        const double n = st[0];
        float* o = RT + (long)b * 12;
        int s8;
        for (int i = 0; i < GDM_POSE_LOSS_REC; ++i) r[i] = 0.0;        // a crop that is not fitted leaves zeros, not leftovers
        bool finite = true;
        for (int i = 0; i < 12; ++i) {
            const float v = RT_gt[(long)b * 12 + i];
            finite = finite && (fabsf(v) <= 3.402823466e38f);
            fit[12 + i] = (double)v;
        }
        if (!(count[b] >= min_points) || !(n > 0.0)) {                  // as kabsch_solve_w_kernel: too few, the sentinel pose
            sentinel_pose(o);
            s8 = 1;
        } else {
            double cBd[3], Sd[3][3];
            {
#include "gdm_kabsch_fit.inc"
                for (int i = 0; i < 3; ++i) {
                    cAd[i] = cA[i]; cBd[i] = cB[i];
                    for (int j = 0; j < 3; ++j) { Rd[i][j] = R[i][j]; Sd[i][j] = S[i][j]; }
                }
            }
            for (int i = 0; i < 3; ++i) {
                double t = cBd[i];                                       // t = cB - R cA in fp64, the fragment's own order
                for (int j = 0; j < 3; ++j) { fit[3 * i + j] = Rd[i][j]; t -= Rd[i][j] * cAd[j]; r[REC_R + 3 * i + j] = Rd[i][j]; }
                fit[9 + i] = t;
                r[REC_CA + i] = cAd[i];
                r[REC_CB + i] = cBd[i];
            }
            r[REC_W] = n;
            s8 = gdm_pose_fit_condition(Rd, Sd, cond_min, lam, V);
            if (!finite) s8 = 1;                                         // no loss against a ground truth that is not a pose
        }
        fit[24] = (double)s8;
        r[REC_STATE] = (double)s8;
    }
    __syncthreads();
    const int s8 = (int)fit[24];
    if (s8 != 0) {                                                      // the whole block leaves together
        if (threadIdx.x == 0) { loss[b] = 0.0; state[b] = (uint8_t)s8; sym_idx[b] = -1; }
        return;
    }
    double pose[12], gt[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) { pose[i] = fit[i]; gt[i] = fit[12 + i]; }

    // D_s = (1/K) sum_k |e_sk|: lanes stride the points, block_sum adds the lanes of a wave by one butterfly and the waves left to right
    double best = 0.0;
    int win = 0;
    for (int s = 0; s < S; ++s) {
        const float* sm = sym ? sym + (long)s * 12 : nullptr;
        double acc[1] = {0.0}, tot[1], e[3];
        for (int k = threadIdx.x; k < K; k += 256) {
            pose_error(pose, gt, sm, model_pts[3 * k], model_pts[3 * k + 1], model_pts[3 * k + 2], e);
            acc[0] += sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        }
        block_sum<1>(acc, red1, tot);
        __syncthreads();                                                // red1 is written again by the next s
        const double D = tot[0] / (double)K;
        if (s == 0 || D < best) { best = D; win = s; }                  // the lowest s wins a tie
    }

    // G = (1/K) sum_k e^ X^T, g = (1/K) sum_k e^ over the winner, e^ = e / |e| (0 where |e| = 0)
    {
        const float* sm = sym ? sym + (long)win * 12 : nullptr;
        double acc[12], tot[12], e[3];
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = 0.0;
        for (int k = threadIdx.x; k < K; k += 256) {
            const double x = model_pts[3 * k], y = model_pts[3 * k + 1], z = model_pts[3 * k + 2];
            pose_error(pose, gt, sm, x, y, z, e);
            const double len = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
            if (!(len > 0.0)) continue;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double u = e[i] / len;
                acc[3 * i] += u * x; acc[3 * i + 1] += u * y; acc[3 * i + 2] += u * z;
                acc[9 + i] += u;
            }
        }
        block_sum<12>(acc, red12, tot);
        if (threadIdx.x == 0) {
            double G[3][3], g[3], Gamma[3][3], Rtg[3];
            for (int i = 0; i < 3; ++i) {
                g[i] = tot[9 + i] / (double)K;
                for (int j = 0; j < 3; ++j) G[i][j] = tot[3 * i + j] / (double)K;
            }
            gdm_pose_fit_adjoint(Rd, cAd, lam, V, G, g, Gamma, Rtg);
            for (int i = 0; i < 3; ++i) {
                r[REC_RTG + i] = Rtg[i];
                r[REC_G + i] = g[i];
                for (int j = 0; j < 3; ++j) r[REC_GAMMA + 3 * i + j] = Gamma[i][j];
            }
            loss[b] = best;
            state[b] = 0;
            sym_idx[b] = win;
        }
    }
}

// grid (B, ceil(N / 1024)): a workgroup takes 1024 consecutive points of its crop, four per lane.
__global__ __launch_bounds__(256) void pose_loss_bwd_kernel(const float* __restrict__ scene_xyz, long scene_bstride, int pt_stride,
                                                            int ch_stride, const float* __restrict__ target,
                                                            const float* __restrict__ weight, const uint8_t* __restrict__ mask,
                                                            const double* __restrict__ rec, const double* __restrict__ grad_loss, int N,
                                                            float* __restrict__ grad_target, float* __restrict__ grad_weight)
{
    const int b = blockIdx.x;
    const double* r = rec + (long)b * GDM_POSE_LOSS_REC;
    const bool fitted = r[REC_STATE] == 0.0;
    const double up = grad_loss[b];
    const double invW = fitted ? 1.0 / r[REC_W] : 0.0;
    const float* sp = scene_xyz + (long)b * scene_bstride;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long i = (long)blockIdx.y * 1024 + q * 256 + threadIdx.x;
        if (i >= N) break;
        const long p = (long)b * N + i;
        float ga[3] = {0.f, 0.f, 0.f}, gw = 0.f;                        // zeros for a skipped point and for a crop that is not fitted
        if (fitted && mask[p]) {
            const float wf = weight[p];
            if (weight_usable(wf)) {
                const double w = wf;
                const double ac[3] = {(double)target[3 * p] - r[REC_CA], (double)target[3 * p + 1] - r[REC_CA + 1],
                                      (double)target[3 * p + 2] - r[REC_CA + 2]};
                const double bc[3] = {(double)sp[i * pt_stride] - r[REC_CB], (double)sp[i * pt_stride + ch_stride] - r[REC_CB + 1],
                                      (double)sp[i * pt_stride + 2 * (long)ch_stride] - r[REC_CB + 2]};
                double dw = 0.0, bg = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double gb = (r[REC_GAMMA + 3 * c] * bc[0] + r[REC_GAMMA + 3 * c + 1] * bc[1]) + r[REC_GAMMA + 3 * c + 2] * bc[2];
                    const double da = gb - r[REC_RTG + c] * invW;        // Gamma (B - cB) - R^T g / W
                    ga[c] = (float)((w * da) * up);
                    dw += ac[c] * da;
                    bg += bc[c] * r[REC_G + c];
                }
                gw = (float)((dw + bg * invW) * up);
            }
        }
        grad_target[3 * p] = ga[0];
        grad_target[3 * p + 1] = ga[1];
        grad_target[3 * p + 2] = ga[2];
        grad_weight[p] = gw;
    }
}

} // namespace

extern "C" size_t gdm_pose_loss_record_bytes(int B)
{
    if (B < 1) return 0;
    return (size_t)B * (16 + GDM_POSE_LOSS_REC) * sizeof(double) + (((size_t)B * sizeof(int32_t) + 7) & ~(size_t)7);
}

extern "C" int gdm_pose_loss_fwd_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* target,
                                     const float* weight, const uint8_t* mask, const float* RT_gt, const float* model_pts,
                                     const float* sym, int B, int N, int K, int S, int min_points, double cond_min, void* record,
                                     size_t record_bytes, double* loss, float* RT, uint8_t* state, int32_t* sym_idx, void* stream)
{
    const char* me = "gdm_pose_loss_fwd_hip";
    const bool ptrs = scene_xyz && target && weight && mask && RT_gt && model_pts && record && loss && RT && state && sym_idx;
    if (int rc = pair_entry_check(me, ptrs, B, N, K, true, scene_bstride, pt_stride, ch_stride, true)) return rc;
    GDM_CHECK_ARG(S >= 1 && S <= GDM_POSE_LOSS_MAX_S, "%s: S=%d symmetry transforms not in [1, %d]", me, S, GDM_POSE_LOSS_MAX_S);
    GDM_CHECK_ARG(sym || S == 1, "%s: S=%d needs the symmetry transforms (NULL is the identity alone)", me, S);
    GDM_CHECK_ARG(cond_min >= 0.0 && cond_min < 1.0, "%s: cond_min=%g not in [0, 1)", me, cond_min);
    GDM_CHECK_ARG(((uintptr_t)record & 7) == 0 && record_bytes >= gdm_pose_loss_record_bytes(B),
                  "%s: the record needs %zu bytes aligned to 8, got %zu", me, gdm_pose_loss_record_bytes(B), record_bytes);
    const RecordViews v = record_views(record, B);
    if (int rc = gdm_kabsch_stats_w_hip(scene_xyz, scene_bstride, pt_stride, ch_stride, nullptr, nullptr, target, weight, mask, B, N, 0,
                                        v.stats, v.count, stream))
        return rc;
    hipLaunchKernelGGL(pose_loss_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, v.stats, v.count, RT_gt, model_pts, sym, K, S,
                       min_points, cond_min, v.rec, loss, RT, state, sym_idx);
    return gdm_launch_status("pose_loss_fwd_kernel");
}

extern "C" int gdm_pose_loss_bwd_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* target,
                                     const float* weight, const uint8_t* mask, const void* record, size_t record_bytes,
                                     const double* grad_loss, int B, int N, float* grad_target, float* grad_weight, void* stream)
{
    const char* me = "gdm_pose_loss_bwd_hip";
    const bool ptrs = scene_xyz && target && weight && mask && record && grad_loss && grad_target && grad_weight;
    if (int rc = pair_entry_check(me, ptrs, B, N, -1, true, scene_bstride, pt_stride, ch_stride, true)) return rc;
    GDM_CHECK_ARG(((uintptr_t)record & 7) == 0 && record_bytes >= gdm_pose_loss_record_bytes(B),
                  "%s: the record needs %zu bytes aligned to 8, got %zu", me, gdm_pose_loss_record_bytes(B), record_bytes);
    GDM_CHECK_ARG(N <= 65535 * 1024, "%s: N=%d > %d", me, N, 65535 * 1024);
    const RecordViews v = record_views(const_cast<void*>(record), B);
    hipLaunchKernelGGL(pose_loss_bwd_kernel, dim3(B, gdm_cdiv(N, 1024)), dim3(256), 0, (hipStream_t)stream, scene_xyz, scene_bstride,
                       pt_stride, ch_stride, target, weight, mask, v.rec, grad_loss, N, grad_target, grad_weight);
    return gdm_launch_status("pose_loss_bwd_kernel");
}
