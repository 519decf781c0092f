/*
 * gdm.h -- C ABI of libgdm_hip.so, the MI355X (gfx950) implementation of the geoMatch
 * dense-correspondence hot path.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every `*_hip` entry point takes DEVICE pointers and a HIP stream (hipStream_t passed
 *     as void*; NULL = the null stream), enqueues its kernels on that stream and returns
 *     without synchronising.  All are re-entrant (no global mutable state), so they can be
 *     driven from several host threads on several streams, as evaluator.py:294-303 does.
 *   - return value: 0 on success, a positive hipError_t, or a negative GDM_E* code.
 *     gdm_last_error() returns a thread-local description of the last failure.
 *   - all tensors are dense, row-major, fp32 unless said otherwise; indices are int32.
 *   - the reference interface each entry point replaces is cited as file:line under
 *     /root/reference.
 */
#ifndef GDM_H
#define GDM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDM_EINVAL (-1)   /* bad argument (shape, K, alignment) */
#define GDM_ENOMEM (-2)   /* workspace too small */

const char* gdm_last_error(void);
/* ABI version, bumped when a signature changes. */
int gdm_version(void);

/* ---------------------------------------------------------------------------------------
 * Exact K-nearest-neighbour search (fp32 squared L2, ascending; ties by ascending index).
 * ------------------------------------------------------------------------------------- */

/* Drop-in for the reference's only native entry point on the live path:
 *   void cpp_knn_batch_omp(const float* batch_data, size_t batch_size, size_t npts, size_t dim,
 *                          const float* queries, size_t nqueries, size_t K, long* batch_indices)
 *   models/RandLA/utils/nearest_neighbors/knn_.h:17-19, knn_.cxx:104-135
 * Same argument list, HOST pointers, caller-allocated output, no return code (as the
 * reference).  Runs on the GPU: H2D copy, gdm_knn_batch_hip, D2H copy, widened to long.
 * dim must be 3.  On failure indices are left untouched and gdm_last_error() is set.   */
void gdm_knn_batch(const float* batch_data, size_t batch_size, size_t npts, size_t dim,
                   const float* queries, size_t nqueries, size_t K, long* batch_indices);

/* Device-resident form. support f32[B,S,3], query f32[B,Q,3] -> idx i32[B,Q,K],
 * d2 f32[B,Q,K] (may be NULL).  1 <= K <= 32.  Slots beyond S (K > S) hold index 0, as the
 * zero-initialised output of knn.pyx:93 does.                                           */
int gdm_knn_batch_hip(const float* support, const float* query, int B, int S, int Q, int K,
                      int32_t* idx, float* d2, void* stream);

/* One launch for a whole table of independent searches (the 22 calls per crop of
 * datasets/lm/linemod_pbr.py:534-569, for all crops of a batch).                        */
typedef struct gdm_knn_job {
    const float* support;     /* f32[B,S,3], batch item b at support + b*support_bstride */
    const float* query;       /* f32[B,Q,3], batch item b at query + b*query_bstride     */
    int32_t* idx;             /* i32[B,Q,K] dense */
    float* d2;                /* f32[B,Q,K] dense, or NULL */
    int64_t support_bstride;  /* in floats; S*3 when dense (0: one support shared by all). A prefix slice cld[:, :S] of a  */
    int64_t query_bstride;    /* [B,N,3] array keeps bstride N*3 (linemod_pbr.py:538)     */
    int32_t S, Q, K;
    int32_t grid_w;           /* 0, or: the support is an ORGANISED map (e.g. the xyz of a depth crop) of S / grid_w rows x grid_w columns
                               * in row-major pixel order -- a hint that lets K > 1 searches with a workspace prune by pixel columns / rows;
                               * results are identical with and without it, for any finite data                                     */
} gdm_knn_job;
#define GDM_KNN_MAX_JOBS 32
/* jobs is a HOST array.  workspace: device memory (16-byte aligned, >= gdm_knn_jobs_workspace_bytes) in which every distinct support
 * set of the K > 1 jobs is re-laid out once: small unorganised supports as hashed float4 tiles that the search blocks stream with
 * coalesced loads, unorganised supports of >= 1024 points as (x, y) cell lists (a counting sort per crop; a query then visits cells
 * ring by ring instead of every point), organised supports (grid_w) as per-column / per-row ratio ranges.  workspace NULL with
 * workspace_bytes 0: each block gathers its tiles from the [S,3] array.  Results are identical in every form, for any data with
 * finite coordinates (the order of NaN and infinite coordinates is not defined and may differ between the forms).
 * Bytes per distinct (support, S, support_bstride, layout), each rounded up to 16, reserved in the order of the jobs by descending S:
 *   ranges (W = grid_w and H = S / grid_w both in [8, 256]):  B * (2 W + 2 H + 2 ceil(H / 16)) * 4
 *   cell list (no ranges, S >= 1024):                         B * S * 16 + B * 1036 * 4
 *   hashed tiles (every other K > 1 job):                     B * ntiles * npad * 16, ntiles = ceil(S / 1024), npad = the power of two
 *                                                             >= max(64, ceil(S / ntiles))
 * gdm_knn_jobs_workspace_bytes is their sum.  With fewer bytes a job whose entry no longer fits takes the next layout of
 * ranges -> cell list (S >= 1024) -> hashed tiles -> gather from the [S,3] array; the results do not change.                     */
size_t gdm_knn_jobs_workspace_bytes(const gdm_knn_job* jobs, int njobs, int B);
int gdm_knn_jobs_ws_hip(const gdm_knn_job* jobs, int njobs, int B, void* workspace, size_t workspace_bytes, void* stream);

/* Ball query (lib/pointops/functions/pointops.py:205-219 `ballquery_cuda(b,n,m,radius,nsample,
 * new_xyz,xyz,idx)`): for each centre the first `nsample` support indices (ascending index)
 * with d2 < radius^2; remaining slots repeat the first hit; all zero when none.
 * xyz f32[B,n,3], new_xyz f32[B,m,3] -> idx i32[B,m,nsample].                           */
int gdm_ballquery_hip(int B, int n, int m, float radius, int nsample,
                      const float* new_xyz, const float* xyz, int32_t* idx, void* stream);

/* Furthest point sampling (pointops.py:40-50 `furthestsampling_cuda(b,n,m,xyz,temp,idx)`):
 * starts from index 0, `temp` f32[B,n] is scratch (initialised inside).                  */
int gdm_furthestsampling_hip(int B, int n, int m, const float* xyz, float* temp, int32_t* idx, void* stream);

/* Three-point interpolation (pointops.py:114-144 `interpolation_forward/backward_cuda`): feat f32[b,c,m], idx i32[b,n,3],
 * weight f32[b,n,3] -> out f32[b,c,n]; backward scatters grad_out f32[b,c,n] into a ZERO-FILLED grad_feat f32[b,c,m].  */
int gdm_interpolation_forward_hip(int B, int c, int m, int n, const float* feat, const int32_t* idx, const float* weight, float* out, void* stream);
int gdm_interpolation_backward_hip(int B, int c, int n, int m, const float* grad_out, const int32_t* idx, const float* weight,
                                   float* grad_feat, void* stream);

/* Label histograms (pointops.py:289-338): label_stat i32[b,n,nclass] summed over the points inside the ball of each centre
 * (`labelstat_ballrange_cuda(b,n,m,radius,nclass,new_xyz,xyz,label_stat,new_label_stat)`) or over idx i32[b,m,nsample]
 * (`labelstat_idx_cuda(b,n,m,nsample,nclass,label_stat,idx,new_label_stat)`) -> i32[b,m,nclass].                        */
int gdm_labelstat_ballrange_hip(int B, int n, int m, float radius, int nclass, const float* new_xyz, const float* xyz,
                                const int32_t* label_stat, int32_t* new_label_stat, void* stream);
int gdm_labelstat_idx_hip(int B, int n, int m, int nsample, int nclass, const int32_t* label_stat, const int32_t* idx,
                          int32_t* new_label_stat, void* stream);

/* ---------------------------------------------------------------------------------------
 * Feature gather / scatter (channel-major features, as the reference network keeps them).
 * ------------------------------------------------------------------------------------- */

/* out[b,c,j,k] = feat[b,c,idx[b,j,k]]   feat f32[B,C,n], idx i32[B,m,K] -> f32[B,C,m,K]
 * replaces Building_block.gather_neighbour + permute (models/RandLA/RandLANet.py:729-738,
 * 704-716) and pointops grouping_forward_cuda (pointops.py:151-176); with K == 1 also
 * FFB6DEmb.nearest_interpolation (models/ffb6d.py:148-163), the `choose` gather
 * (ffb6d.py:278-281) and pointops gathering_forward_cuda (pointops.py:61-82).              */
int gdm_group_gather_hip(const float* feat, const int32_t* idx, int B, int C, int n, int m, int K,
                         float* out, void* stream);
/* grad_feat[b,c,idx[b,j,k]] += grad_out[b,c,j,k]; grad_feat must be zeroed by the caller.  grad_out may be read in place from a
 * wider tensor: go_bstride = floats between two batch items (rows of m*K floats, channel stride m*K; >= C*m*K, C*m*K when dense)
 * -- the gradient slice a torch.cat backward hands to nearest_interpolation (models/ffb6d.py:148-163) */
int gdm_group_gather_bwd2_hip(const float* grad_out, long go_bstride, const int32_t* idx, int B, int C, int n, int m, int K,
                              float* grad_feat, void* stream);

/* out[b,c,j] = max_k feat[b,c,idx[b,j,k]]; arg i32[B,C,m] (may be NULL) = winning source index.
 * replaces FFB6DEmb.random_sample (models/ffb6d.py:128-146).                             */
int gdm_gather_max_hip(const float* feat, const int32_t* idx, int B, int C, int n, int m, int K,
                       float* out, int32_t* arg, void* stream);
/* grad_feat[b,c,arg[b,c,j]] += grad_out[b,c,j]; grad_feat zeroed by the caller.          */
int gdm_gather_max_bwd_hip(const float* grad_out, const int32_t* arg, int B, int C, int n, int m,
                           float* grad_feat, void* stream);

/* Relative position encoding (RandLANet.py:720-727 + the permute of :701-702):
 * xyz f32[B,n,3], idx i32[B,n,K] -> out f32[B,10,n,K] with channels
 * [ |p_i-p_j|, p_i-p_j (3), p_i (3), p_j (3) ].                                          */
int gdm_rel_pos_enc_hip(const float* xyz, const int32_t* idx, int B, int n, int K, float* out, void* stream);

/* Attentive pooling core (RandLANet.py:749-752): softmax of `att` over K, weighted sum of
 * `feat` over K.  att, feat f32[B,C,n,K] -> out f32[B,C,n].                              */
int gdm_att_pool_hip(const float* att, const float* feat, int B, int C, int n, int K, float* out, void* stream);
int gdm_att_pool_bwd_hip(const float* att, const float* feat, const float* grad_out, int B, int C, int n, int K,
                         float* grad_att, float* grad_feat, void* stream);

/* ---------------------------------------------------------------------------------------
 * N x M descriptor matching (cosine similarity + row arg-max).
 * ------------------------------------------------------------------------------------- */

#define GDM_MATCH_BF16X3 0   /* split-bf16 MFMA: hi*hi + hi*lo + lo*hi, fp32 accumulate (|err| <= ~1.2e-5) */
#define GDM_MATCH_F32    1   /* f32-input MFMA, exact fp32 products                                        */

/* Workspace bytes needed by gdm_match_hip for the given sizes. */
size_t gdm_match_workspace_bytes(int B, int N, int M);

/* Fused inference matching (evaluator.py:87-93): L2-normalise each scene descriptor (over D),
 * each model descriptor (over D), similarity = scene . model, per scene point the maximum
 * over the M model vertices and its index (first maximum on exact ties).
 *   scene f32[B,D,N] channel-major (GeoMatch end_points['rgbd'], geoMatch.py:199)
 *   model f32[D,M]   channel-major (end_points['mesh'][0])
 *   -> best_idx i32[B,N], best_sim f32[B,N]; sim f32[B,N,M] is also written when non-NULL
 *      (the materialised matrix of evaluator.py:91).
 * D must be 128; B, N, M arbitrary (an (M+1)-column padded model, geoMatch.py:117-119, works).
 * = gdm_match_pack_hip(scene) + gdm_match_pack_hip(model) + gdm_match_packed_hip.            */
int gdm_match_hip(const float* scene, const float* model, int B, int D, int N, int M, int precision,
                  int32_t* best_idx, float* best_sim, float* sim,
                  void* workspace, size_t workspace_bytes, void* stream);

/* The two stages separately, so that an object's model rows are packed once and reused
 * (they are constant in eval: models/SplineCNN.py:234 takes no input).
 * pack: x f32[R,D,n] channel-major -> R*n normalised rows of 512 bytes (gdm_match_rows_bytes(R*n)). */
size_t gdm_match_rows_bytes(int rows);
size_t gdm_match_partial_bytes(int B, int N);
int gdm_match_pack_hip(const float* x, int R, int D, int n, int precision, void* rows, void* stream);
/* two packs in one launch (the scene and the model descriptors of one step; evaluator.py:80-81 normalises both): the same bytes as
 * gdm_match_pack_hip(x1, R1, D, n1, ..., rows1) + gdm_match_pack_hip(x2, R2, D, n2, ..., rows2) */
int gdm_match_pack2_hip(const float* x1, int R1, int n1, void* rows1, const float* x2, int R2, int n2, void* rows2,
                        int D, int precision, void* stream);
/* scene_rows, model_rows and partial must be 16-byte aligned (also for gdm_match_soft_packed_hip). */
int gdm_match_packed_hip(const void* scene_rows, const void* model_rows, int R /* B*N */, int M, int precision,
                         int32_t* best_idx, float* best_sim, float* sim,
                         void* partial, size_t partial_bytes, void* stream);

/* Soft assignment on the same similarities (sim_ij = s_i . m_j in the kernel's own arithmetic), gamma a temperature:
 *   lse_i      = log sum_j exp(gamma sim_ij)                      f32[R]
 *   conf_i     = exp(gamma best_sim_i - lse_i)                    f32[R]     in (0, 1]: softmax probability of the arg-max vertex
 *   soft_xyz_i = sum_j exp(gamma sim_ij - lse_i) model_xyz_j      f32[R,3]   expected model coordinate (model_xyz f32[M,3])
 * over exactly the M real columns and for every row; best_idx / best_sim are those of gdm_match_packed_hip on the same rows, bit
 * for bit.  No [R, M] tensor is written and no atomic is used: the kernel accumulates exp(gamma (sim - 1)) (cosines are <= 1, so
 * the fixed shift 1 needs no running maximum, and gamma <= 40 keeps every term >= e^-80, a normal fp32), one partial per 256-column
 * panel and row goes to `partial` (gdm_match_soft_partial_bytes(B, N), 16-byte aligned) and the panels are added in ascending
 * order, so two runs are bit-identical.  0 < gamma <= GDM_MATCH_SOFT_MAX_GAMMA and 1 <= M <= GDM_MATCH_SOFT_MAX_M (the 64 panels
 * the LDS-resident kernel form covers); anything else, a NaN gamma included, is refused with GDM_EINVAL before any launch. */
#define GDM_MATCH_SOFT_MAX_GAMMA 40.0f
#define GDM_MATCH_SOFT_MAX_M     16384
size_t gdm_match_soft_partial_bytes(int B, int N);
int gdm_match_soft_packed_hip(const void* scene_rows, const void* model_rows, const float* model_xyz, int R /* B*N */, int M,
                              int precision, float gamma, int32_t* best_idx, float* best_sim, float* lse, float* conf,
                              float* soft_xyz, void* partial, size_t partial_bytes, void* stream);
/* score f32[B] = the mean of conf f32[B,N] over the points with mask u8[B,N] != 0, 0 for a crop with none (fp64, fixed order): the
 * number an estimate is ranked by (the `score` column of a BOP csv). */
int gdm_match_score_hip(const float* conf, const uint8_t* mask, int B, int N, float* score, void* stream);

/* THE TWO-WAY RULE.  Matching in both directions from one pass over the similarities.  scene_rows: B*N packed rows (crop b owns rows
 * b*N .. b*N+N-1), model_rows: M packed rows, mask u8[B,N]; sim_ij is the kernel's own similarity (the arithmetic of
 * gdm_match_packed_hip at that precision).
 *   best_idx i32[B,N], best_sim f32[B,N]   those of gdm_match_packed_hip on the same rows, bit for bit, for every row, masked or not
 *   col_idx i32[B,M], col_sim f32[B,M]     per crop b and vertex j: start from (idx, sim) = (-1, -inf) and let a point i of the crop
 *                                          with mask[b,i] != 0 take over iff sim_ij > sim (the comparison of the row arg-max: a NaN
 *                                          never wins), the lowest such i on exact ties; i counts inside the crop, 0 .. N-1
 * so a crop with no masked point, or a column whose masked similarities are all NaN, gives col_idx = -1 and col_sim = -inf.  A
 * winning similarity of -0 is reported as +0 (the two compare equal).
 * No [R, M] tensor and no floating-point atomic: a lane reduces its column over its 16 rows, the two half-waves merge by shuffle,
 * and the waves, the row blocks and the crops a row block spans merge through an integer maximum of the 64-bit key
 * (order-preserving image of sim << 32 | ~i), which is exact and commutes: two launches give the same bytes.  The keys live in
 * `partial` (gdm_match_twoway_partial_bytes(B, N, M), 16-byte aligned) behind the row partials and are reset inside the call, so the
 * result does not depend on what `partial` held.  1 <= M <= GDM_MATCH_SOFT_MAX_M (the 64 panels of the LDS-resident kernel form);
 * that, a NULL argument, a non-positive size, a bad precision or rows off a 16-byte boundary is refused with GDM_EINVAL before any
 * launch. */
size_t gdm_match_twoway_partial_bytes(int B, int N, int M);
int gdm_match_twoway_packed_hip(const void* scene_rows, const void* model_rows, const uint8_t* mask, int B, int N, int M, int precision,
                                int32_t* best_idx, float* best_sim, int32_t* col_idx, float* col_sim, void* partial,
                                size_t partial_bytes, void* stream);
/* THE CYCLE RULE.  Scene xyz addressed as in gdm_kabsch_stats_hip; best_idx i32[B,N], col_idx i32[B,M], mask u8[B,N]; radius finite
 * and >= 0 (else GDM_EINVAL).  For a point i of crop b with mask != 0: j = best_idx[b,i], k = col_idx[b,j], d = p_i - p_k (fp32,
 * component by component), d2 = ((dx*dx) + dy*dy) + dz*dz in fp32, every product and sum rounded on its own (no contraction); the
 * point is kept iff d2 <= radius*radius (the product in fp32).  k == i gives d2 = 0, so radius = 0 keeps exactly the mutual best
 * pairs (and the points that coincide with their vertex's point).  j outside [0,M), k outside [0,N) or a NaN d2 drops the point.
 *   pair_mask u8[B,N]; pair_count i32[B] = the kept points of the crop (written, not accumulated);
 *   cycle_d2 f32[B,N] = d2 where one was formed (a NaN included, of whatever sign and payload the arithmetic gives it), +inf where
 *   the point is unmasked or dropped without one. */
int gdm_match_cycle_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const int32_t* best_idx,
                        const int32_t* col_idx, const uint8_t* mask, int B, int N, int M, float radius, uint8_t* pair_mask,
                        int32_t* pair_count, float* cycle_d2, void* stream);
/* THE DUAL RULE.  Soft matching in both directions from one pass over the similarities: the row softmax of
 * gdm_match_soft_packed_hip, the column arg-max of gdm_match_twoway_packed_hip and the column softmax under the mask, whose product
 * with the row softmax is the dual-softmax confidence of a pair.  Inputs as those two entries take them: B*N packed scene rows, M
 * packed model rows, model_xyz f32[M,3], mask u8[B,N], 0 < gamma <= GDM_MATCH_SOFT_MAX_GAMMA.  With k2 = gamma * log2(e) in fp32,
 * w_ij = exp2(fma(sim_ij, k2, -k2)): the soft kernel's own two instructions on the same similarity bits.
 *   best_idx, best_sim, lse, conf, soft_xyz   those of gdm_match_soft_packed_hip, bit for bit, for every row, masked or not
 *   col_idx i32[B,M], col_sim f32[B,M]        those of gdm_match_twoway_packed_hip, bit for bit
 *   Zc[b,j]  (in `partial`)                   the sum of w_ij over the points i of crop b with mask != 0, in fp32 and a fixed order
 *   col_lse f32[B,M]  = gamma + log Zc        the logarithm in fp64; -inf where the crop has no masked point
 *   col_conf f32[B,M] = w(col_sim) / Zc       w recomputed by the same two instructions, the quotient in fp64; 0 where col_idx = -1.
 *                                             The share of the column that the vertex's best point holds, in (0, 1]
 *   dual f32[B,N]     = conf_i * (w_ij / Zc[b,j]) at j = best_idx[i] for a point with mask != 0, from best_sim's and conf's fp32
 *                                             values, quotient and product in fp64, rounded once; 0 for any other point
 * Point i is one of Zc's terms and fp32 addition of non-negative terms is monotone, so w_ij <= Zc and 0 <= dual <= conf <= 1.
 * The order of Zc: the rows are cut into blocks of 256 that start at each crop's first row (none spans a crop); inside a block a
 * lane adds its 16 rows in ascending order, the two half-waves add by one shuffle, the 8 waves are added in ascending order, and
 * the blocks of a crop in ascending order.  No [R, M] tensor, no floating-point atomic: two launches give the same bytes.  The
 * workspace `partial` (gdm_match_dual_partial_bytes(B, N, M), 16-byte aligned) holds the soft launch's partials, the two-way
 * launch's keys (reset inside the call), one column partial per row block and Zc; the result does not depend on what it held.
 * Limits: those of both entries (B*N < 2^22, 1 <= M <= GDM_MATCH_SOFT_MAX_M); they, a NULL argument, a non-positive size, a bad
 * precision, a gamma outside its range (a NaN included) or rows off a 16-byte boundary are refused with GDM_EINVAL before any launch. */
size_t gdm_match_dual_partial_bytes(int B, int N, int M);
int gdm_match_dual_packed_hip(const void* scene_rows, const void* model_rows, const float* model_xyz, const uint8_t* mask, int B, int N,
                              int M, int precision, float gamma, int32_t* best_idx, float* best_sim, float* lse, float* conf,
                              float* soft_xyz, int32_t* col_idx, float* col_sim, float* col_lse, float* col_conf, float* dual,
                              void* partial, size_t partial_bytes, void* stream);

/* seg f32[B,2,N] -> mask u8[B,N] = (argmax over the 2 classes == 1) (evaluator.py:79-83),
 * count i32[B] of selected points (zeroed inside).                                        */
int gdm_seg_mask_hip(const float* seg, int B, int N, uint8_t* mask, int32_t* count, void* stream);

/* ---------------------------------------------------------------------------------------
 * SplineConv sparse part for the object-model branch (models/SplineCNN.py:136-140,234-239;
 * arithmetic of the un-vendored torch_spline_conv, dim=3, degree 1, open splines, mean aggr).
 * xw f32[M, ks^3, C] = X @ [W_0|...|W_{ks^3-1}] (dense GEMM done by the caller),
 * CSR edges sorted by target: rowptr i32[M+1], src i32[E], attr f32[E,3] in [0,1],
 * root f32[M,C] (x W_root) or NULL, bias f32[C] or NULL -> out f32[M,C] (optional ReLU).     */
int gdm_spline_aggregate_hip(const float* xw, const int32_t* rowptr, const int32_t* src, const float* attr,
                             const float* root, const float* bias, int M, int C, int kernel_size, int relu,
                             float* out, void* stream);
/* grad_xw[src, wi_s, :] += b_s * grad_out[target, :] / deg(target); grad_xw zeroed by the caller. */
int gdm_spline_aggregate_bwd_hip(const float* grad_out, const int32_t* rowptr, const int32_t* src, const float* attr,
                                 int M, int C, int kernel_size, float* grad_xw, void* stream);
/* The same layer for few input channels (Cin <= 16; the first mesh layer, 9 -> 128) without the [M, 125*C] table:
 * out_i = mean_e sum_s b_s (x_j . W[wi_s]) + x_i . W_root + bias; x f32[M,Cin], weight f32[ks^3,Cin,C] (SplineConv.weight as stored),
 * root_t f32[Cin,C] (lin.weight transposed, may be NULL), bias f32[C] (may be NULL).
 * This kernel and gdm_spline_pairs_aggregate3_hip write up to three forms of the result: out f32[M,C]; out_t f32[C,M] (channel-major:
 * what the next layer's grouped GEMM, its root product and the final linear read as gdm_pointwise2_hip segments); out_packed, the
 * split-bf16 operand planes of the next layer's grouped GEMM (gdm_conv3x3_act_bytes(1, C, 1, M) bytes, the layout
 * gdm_conv3x3_pack_act_hip(x_cm, 1, C, 1, M) writes; zero border in place, C = 128, 256 or 512), so that the pack launch between two
 * SplineConv layers (SplineCNN.py:238-239) is not needed.  Each may be NULL, but not both out and out_t; out_t and out_packed need
 * C % 4 == 0, 512 % C == 0 and 16-byte aligned buffers.
 * weights_in_lds != 0: where it applies (C = 128, kernel_size = 5, the 16-byte path) a workgroup owns 16 output channels and a run of
 * vertices and reads its slice of the weight table, [125][Cin][16] (72,000 B at Cin = 9), from LDS instead of fetching every weight row
 * from L2 once per (edge, corner); 0: always the kernel that reads the table in global memory.  Same arithmetic, same bits. */
int gdm_spline_direct3_hip(const float* x, const float* weight, const int32_t* rowptr, const int32_t* src, const float* attr,
                           const float* root_t, const float* bias, int M, int Cin, int C, int kernel_size, int relu,
                           float* out, float* out_t, void* out_packed, int weights_in_lds, void* stream);
/* Edge-grouped form of the 128-channel layers: only the (source vertex, kernel index) pairs that some edge needs are multiplied,
 * 4x fewer FLOPs than the dense form and no [M, 125*C] table.  gdm_gemm_grouped_hip: Y[r, 0:128] = Wpk[tile_co0[r/256] + 0:128, :] .
 * X[rowidx[r], :] for R % 256 == 0 rows (pairs sorted by kernel index, groups padded to 256 rows with rowidx = 0), X packed by
 * gdm_conv3x3_pack_act_hip(x^T, 1, Cin, 1, M), weights by gdm_conv1x1_pack_weight_hip (125*C rows, row = wi*C + co).
 * The packed X, gdm_conv3x3_act_bytes(1, Cin, 1, M) bytes, and the packed weights must each stay below 2 GiB (the operand limit, at
 * gdm_conv3x3_packed_hip below): refused on the host otherwise.
 * gdm_spline_pairs_aggregate3_hip: out_i = mean_e sum_s basis[e,s] * Y[pos[e,s]] + root_i + bias; root f32[M,C] and bias f32[C] may
 * be NULL. */
int gdm_gemm_grouped_hip(const void* xpk, const void* wpk, const int32_t* rowidx, const int32_t* tile_co0, int R, int M,
                         int Cin, int Cout_total, float* out, void* stream);
int gdm_spline_pairs_aggregate3_hip(const float* Y, const int32_t* rowptr, const int32_t* pos, const float* basis,
                                    const float* root, const float* bias, int M, int C, int relu, float* out, float* out_t,
                                    void* out_packed, void* stream);
/* Training on the edge-grouped form: the backward of gdm_gemm_grouped_hip + gdm_spline_pairs_aggregate3_hip, no [M, 125*C] table, no
 * atomics (every sum in a fixed order).  Static inverse maps of the pairs: pair_ptr i32[R+1] / pair_ec i32[8E] (the (edge, corner) uses
 * e*8+s of every pair row, ascending; padding rows empty), tgt i32[E] (target vertex of every edge), inv_deg f32[M] (1 / in-degree),
 * src_ptr i32[M+1] / src_rows i32[U] (the pair rows of every source vertex, ascending), blk_start / blk_rows i32[nk] (first row and
 * row count of every kernel index' block, padding excluded).
 * gdm_spline_pairs_grad_hip: gy[r, :] = sum_{(e,s) in pair r} basis[e,s] * inv_deg[tgt e] * g[tgt e, :], g = grad_out masked by
 *   out_mask > 0 (the layer's output f32[M,C], ReLU layers) or grad_out itself (out_mask NULL); every one of the R rows is written.
 *   gy f32[R,C]; gy_packed (may be NULL): the same as the packed split-bf16 operand of a [1,C,1,R] map (gdm_conv3x3_act_bytes bytes, zero
 *   border kept by the caller) for the input-gradient GEMM  Z = gdm_gemm_grouped_hip(gy_packed, W packed from weight.reshape(nk*Cin, C),
 *   rowidx = 0..R-1, tile_co0 = k*Cin).
 * gdm_spline_segment_sum_hip: dx[j, :] = add[j, :] (add may be NULL) + sum_{r in src_rows[src_ptr[j] : src_ptr[j+1]]} z[r, :].
 * gdm_spline_wgrad_hip: dw[k] f32[Cin,C] = sum_{r in block k} x[rowidx[r], :]^T gy[r, :] for all nk kernel indices on the exact-fp32
 *   MFMA (v_mfma_f32_32x32x2_f32): one launch forms the partial product of every 256-row tile (tile_co0 i32[R/256] = k*C names its
 *   kernel index) in part f32[R/256, Cin, C] (workspace, no initialisation needed), a second adds each kernel index' partials in
 *   ascending tile order.  x f32[M,Cin], Cin = 128 or <= 32, C = 128; empty blocks are written as zeros. */
int gdm_spline_pairs_grad_hip(const float* grad_out, const float* out_mask, const int32_t* pair_ptr, const int32_t* pair_ec,
                              const float* basis, const int32_t* tgt, const float* inv_deg, int R, int C, float* gy,
                              void* gy_packed, void* stream);
int gdm_spline_segment_sum_hip(const float* z, const int32_t* src_ptr, const int32_t* src_rows, const float* add, int M, int C,
                               float* dx, void* stream);
int gdm_spline_wgrad_hip(const float* x, const int32_t* rowidx, const float* gy, const int32_t* tile_co0, const int32_t* blk_start,
                         const int32_t* blk_rows, int nk, int R, int Cin, int C, float* part, float* dw, void* stream);

/* ---------------------------------------------------------------------------------------
 * Bilinear resize, align_corners=True, NCHW fp32 (models/cnn/pspnet.py:26-29,38).
 * in f32[planes,H,W] -> out f32[planes,OH,OW]; planes = B*C.  Backward writes every element of grad_in
 * (gather form: no atomics, deterministic).                                             */
int gdm_upsample_bilinear_hip(const float* in, long planes, int H, int W, int OH, int OW, float* out, void* stream);
int gdm_upsample_bilinear_bwd_hip(const float* grad_out, long planes, int H, int W, int OH, int OW, float* grad_in, void* stream);

/* ---------------------------------------------------------------------------------------
 * DGCNN variant (models/dgcnn.py, models/geoMatch_DGCNN.py).
 * top-k per row of a dense score matrix (dgcnn.py:21-27 `pairwise_distance.topk(k)`): score f32[rows,n]
 * -> idx i32[rows,K] (descending score, ties by ascending column), val f32[rows,K] or NULL.  K <= 32.
 * edge feature (dgcnn.py:30-56): x f32[B,C,n], idx i32[B,n,K] -> out f32[B,2C,n,K] = cat(x_j - x_i, x_i). */
int gdm_topk_rows_hip(const float* score, long rows, int n, int K, int32_t* idx, float* val, void* stream);
/* The same top-k over dgcnn.py:22-25's pairwise_distance without materialising it: gram f32[B,n,n] = X^T X, xx f32[B,n] = sum_c x^2;
 * ranks ((-xx[c]) - (-2*gram[r][c])) - xx[r] formed with torch's operations in torch's order (bit-identical indices). */
int gdm_topk_negdist_hip(const float* gram, const float* xx, int B, int n, int K, int32_t* idx, void* stream);
int gdm_edge_feature_hip(const float* x, const int32_t* idx, int B, int C, int n, int K, float* out, void* stream);
int gdm_edge_feature_bwd_hip(const float* grad_out, const int32_t* idx, int B, int C, int n, int K, float* grad_x, void* stream);
/* The fused inference path of the variant: neither the [B,n,n] distances nor the [B,2C,n,K] edge tensor exist.
 * feature_knn (dgcnn.py:21-27 as ONE operator): x f32[B,C,n] channel-major (item b at x + b * x_bstride, rows contiguous) ->
 * idx i32[B,n,K], val f32[B,n,K] or NULL, of the K largest  ((-xx[c]) - (-2 g[r][c])) - xx[r]  per row r, g = x^T x with exact fp32
 * products accumulated in fp32 (fp32 MFMA), xx[c] = sum_ch x[ch][c]^2.  Descending score, ties by ascending column, a row with fewer
 * than K candidates is filled with index 0.  The only workspace is O(B n): xx and one flag per 32 rows (gdm_feature_knn_workspace_bytes);
 * Gram tiles live in registers.  1 <= K <= 32, C <= 128 (a workgroup keeps all channels of its rows in LDS), C * n < 2^29.
 * splits: over how many waves a row group's columns are divided (1, 2 or 4; their lists are merged through LDS), 0 = chosen from
 * the number of workgroups so that one large item still fills the chip.  The result does not depend on it.
 * Deterministic (no atomics on floats; the result does not depend on scheduling). */
size_t gdm_feature_knn_workspace_bytes(int B, int n);
int gdm_feature_knn_hip(const float* x, long x_bstride, int B, int C, int n, int K, int splits, void* ws, size_t ws_bytes, int32_t* idx,
                        float* val, void* stream);
/* edge_block: one edge-convolution stage (dgcnn.py:108-120: get_graph_feature -> conv -> BN -> LeakyReLU [-> conv -> BN -> LeakyReLU]
 * -> max over the neighbours) from the per-point products of its first convolution: pq f32[B,n,128] point-major, columns 0..63 =
 * W_a x, 64..127 = (W_b - W_a) x for W = [W_a | W_b] (W cat(x_j - x_i, x_i) = W_a x_j + (W_b - W_a) x_i).  Per point i:
 *   out[b, out_c0 + c, i] = max_k act2(act1(scale1 (pq[idx[b,i,k], 0:64] + pq[i, 64:128]) + shift1)),   act = LeakyReLU(slope),
 *   act2(h) = LeakyReLU(scale2 (w2 h) + shift2) with w2 f32[64,64] as the convolution holds it, or the identity when w2, scale2 and
 * shift2 are NULL (the single-convolution stage).  out f32[B,out_C,n]; only channels [out_c0, out_c0 + 64) are written.
 * idx i32[B,n,K], clamped to [0, n); 1 <= K <= 32.  pq, scale1, shift1 and w2 must be 16-byte aligned. */
int gdm_edge_block_hip(const float* pq, const int32_t* idx, const float* scale1, const float* shift1, const float* w2, const float* scale2,
                       const float* shift2, float slope, int B, int n, int K, float* out, int out_C, int out_c0, void* stream);
/* edge_block in training mode (train-mode BatchNorm over all E = B n K edges, differentiable): the passes around gdm_edge_block_hip.
 * Every pass recomputes its edges from pq, idx and per-channel numbers; none allocates O(B n K C).  With y1 = pq[idx[b,i,k], 0:64] +
 * pq[i, 64:128], h1 = act(scale1 y1 + shift1), y2 = w2 h1:
 *   st  f32[4][64] per BatchNorm: scale = gamma rstd | shift = beta - mean scale | mean | rstd (of the batch)
 *   cf  f32[2][64] per BatchNorm: dbeta / E | dgamma / E
 *   part f64[gdm_edge_train_groups(B, n)][64][2]: one pair of per-channel sums per workgroup, to be added by the caller (in fp64, in a
 *        fixed order: the sums do not depend on scheduling)
 * gdm_edge_stats_hip       pair = (sum y1, sum y1^2) with st1 = w2 = NULL, else (sum y2, sum y2^2)
 * gdm_edge_bwd_reduce_hip  the last layer's first arg-max over k per (point, channel) -> amax u8[B,n,64], and pair = (dbeta, dgamma) of
 *                          the last BatchNorm (w2 = st2 = NULL: the single-convolution stage); grad_out f32[B,64,n]
 * gdm_edge_bwd_mid_hip     two convolutions: dy2 = scale2 (dz2 - cf2[0] - y2_hat cf2[1]); dw_slabs f32[groups][64][64] = the workgroup's
 *                          sum over its edges of dy2 (x) h1 (fp32 MFMA with the edges as the contraction), pair = (dbeta1, dgamma1)
 * gdm_edge_bwd_scatter_hip dy1 = scale1 (dz1 - cf1[0] - y1_hat cf1[1]) -> grad_pq f32[B,n,128]: columns 0..63 of row idx[b,i,k] by
 *                          atomicAdd (ZEROED by the caller; one 256-byte row per edge), columns 64..127 of row i stored
 * idx is clamped to [0, n) as gdm_edge_block_hip clamps; 1 <= K <= 32; pq, st1 and w2 16-byte aligned. */
long gdm_edge_train_groups(int B, int n);
int gdm_edge_stats_hip(const float* pq, const int32_t* idx, const float* st1, const float* w2, float slope, int B, int n, int K, double* part,
                       void* stream);
int gdm_edge_bwd_reduce_hip(const float* pq, const int32_t* idx, const float* st1, const float* w2, const float* st2, float slope, int B, int n,
                            int K, const float* grad_out, uint8_t* amax, double* part, void* stream);
int gdm_edge_bwd_mid_hip(const float* pq, const int32_t* idx, const float* st1, const float* w2, const float* st2, const float* cf2, float slope,
                         int B, int n, int K, const float* grad_out, const uint8_t* amax, double* part, float* dw_slabs, void* stream);
int gdm_edge_bwd_scatter_hip(const float* pq, const int32_t* idx, const float* st1, const float* cf1, const float* w2, const float* st2,
                             const float* cf2, float slope, int B, int n, int K, const float* grad_out, const uint8_t* amax, float* grad_pq,
                             void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused circle loss rows for the training matching (models/geoMatch.py:55-83 matching_loss,
 * models/loss.py:441-494 CircleLoss): positive mask evaluated on the fly, two masked LSEs online.
 * sim f32[R, M+1] (all selected points of the batch, concatenated), match i32[R] (ground-truth vertex, M = none),
 * item i32[R] (batch item of the row), xyz f32[M,3], vis u8[B,M], radius / gamma / m scalars
 * -> lse_p, lse_n, loss f32[R] (loss = softplus(lse_p + lse_n)).
 * Backward: grad_rows f32[R] -> dsim f32[R, M+1].                                             */
int gdm_circle_rows_fwd_hip(const float* sim, int R, int Mp, const int32_t* match, const int32_t* item,
                            const float* xyz, const uint8_t* vis, float radius, float gamma, float m,
                            float* lse_p, float* lse_n, float* loss, void* stream);
int gdm_circle_rows_bwd_hip(const float* sim, int R, int Mp, const int32_t* match, const int32_t* item,
                            const float* xyz, const uint8_t* vis, float radius, float gamma, float m,
                            const float* lse_p, const float* lse_n, const float* grad_rows, float* dsim, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training matching loss without the similarity matrix (gdm_circle.hip): replaces models/geoMatch.py:117-136 (normalise, padded
 * matmul), :55-83 / :86-100 (positive masks) and models/loss.py:441-494 (CircleLoss) and their autograd backward for all selected
 * points of a batch.  x f32[R,128] / y f32[M,128] are UNIT rows (F.normalize stays with the caller's autograd).
 *   pack      x -> split-bf16 rows + d-major tiles + row sums (sizes from the two *_bytes functions, rows padded to 128)
 *   nbr       bit table [M][ceil(M/32)] of vertices within `radius` of each vertex (basic_utils.py:86-89 arithmetic); once per model
 *   visbits   visible_flag u8[B,M] -> bits [B][ceil(M/32)]
 *   fwd2      per-row lse_p, lse_n, loss f32[Rp]; g i32[Rp] = ground-truth vertex (M = none), item i32[Rp]; symmetric objects:
 *             g / c2 = the two positive columns of the row (geoMatch.py:91-95), nbr / visb unused
 *   bwd2      coef f32[Rp] = upstream gradient x sigmoid(lse_p + lse_n) (0 for padding rows and empty positive sets) ->
 *             gx f32[Rp,128], gy_part f32[P][Mp,128] with P = gdm_circle_match_bwd_parts (sum over P = gradient w.r.t. y)
 * fwd2 / bwd2 options: nbr_per_item = 0 -- `nbr` is the one table of gdm_circle_match_nbr_hip; != 0 -- `nbr` holds one neighbour
 * table PER BATCH ITEM, u32[B][M][ceil(M/32)], made by gdm_circle_match_nbr_items_hip from a per-item, per-vertex radius (the
 * geoMatch_DGCNN variant, /root/reference/models/geoMatch_DGCNN.py:52-135; positive_r / 1000 * z of the posed vertex, :66-67).
 * pad_e0 = 0 -- `xpad` holds the row sums that pack wrote; != 0 -- the padding column is the unit vector e0 (geoMatch_DGCNN.py:96-99)
 * and `xpad` holds x[r][0].                                                                                                       */
size_t gdm_circle_match_rows_bytes(int n);
size_t gdm_circle_match_tp_bytes(int n);
/* rows / tp (and xrows, xtp, yrows, ytp below) must be 16-byte aligned. */
int gdm_circle_match_pack_hip(const float* x, int n, void* rows, void* tp, float* rowsum, void* stream);
int gdm_circle_match_nbr_hip(const float* xyz, int M, float radius, uint32_t* nbr, void* stream);
int gdm_circle_match_visbits_hip(const uint8_t* vis, int B, int M, uint32_t* bits, void* stream);
int gdm_circle_match_nbr_items_hip(const float* xyz, int M, const float* rad /* f32[B,M] */, int B, uint32_t* nbr, void* stream);
int gdm_circle_match_fwd2_hip(const void* xrows, const void* xtp, const float* xpad, const void* yrows, const void* ytp,
                              int R, int M, const int32_t* g, const int32_t* c2, const int32_t* item,
                              const uint32_t* nbr, int nbr_per_item, const uint32_t* visb, int pad_e0, float gamma, float m,
                              float* lse_p, float* lse_n, float* loss, void* stream);
int gdm_circle_match_bwd2_hip(const void* xrows, const void* xtp, const float* xpad, const void* yrows, const void* ytp,
                              int R, int M, const int32_t* g, const int32_t* c2, const int32_t* item,
                              const uint32_t* nbr, int nbr_per_item, const uint32_t* visb, int pad_e0, float gamma, float m,
                              const float* lse_p, const float* lse_n, const float* coef, float* gx, float* gy_part, void* stream);
int gdm_circle_match_bwd_parts(int R, int M);

/* ---------------------------------------------------------------------------------------
 * Differentiable soft assignment without the similarity matrix (gdm_softcoord.hip): the training half of the soft matching above.
 * Operands are the buffers gdm_circle_match_pack_hip writes for the UNIT rows x f32[R,128] (xrows, xtp) and y f32[M,128] (yrows,
 * ytp); xyz f32[M,3].  With s_rc = x_r . y_c (split-bf16 products, fp32 accumulation), over exactly the M real columns:
 *   fwd    Z_r = sum_c exp(gamma (s_rc - 1));  lse f32[R]: lse_r = gamma + log Z_r;
 *          soft f32[R,3]: soft_r = sum_c exp(gamma (s_rc - 1)) xyz_c / Z_r
 *   bwd    lse f32[R] of fwd, kb f32[R,4] = (k_r, b_r) with a_r = dL/dlse_r, b_r = dL/dsoft_r, k_r = a_r - b_r . soft_r;
 *          p_rc = exp(gamma s_rc - lse_r), G_rc = dL/ds_rc = gamma p_rc (k_r + b_r . xyz_c);
 *          gx f32[R,128]: gx_r = sum_c G_rc y_c;  gy f32[M,128]: gy_c = sum_r G_rc x_r (no gradient for xyz).
 *          gy_part f32[P][Mp,128] is workspace, Mp = M rounded up to 128, P = parts(R, M): partial sums over slices of the rows,
 *          added in ascending P.  No atomics: two runs are bit-identical.
 *          gx or gy may be NULL (not both): that gradient's launches are skipped (gy_part is needed with gy only).
 * Padded columns weigh nothing and padded rows add nothing, whatever lies beyond R in the caller's buffers (those are not read).
 * 0 < gamma <= GDM_SOFT_COORD_MAX_GAMMA (every term >= e^-80, a normal fp32: the fixed shift 1 needs no running maximum);
 * anything else, a NaN included, is refused with GDM_EINVAL before any launch, and so are packed rows, kb, gy_part or gy off a
 * 16-byte boundary. */
#define GDM_SOFT_COORD_MAX_GAMMA 40.0f
int gdm_soft_coord_fwd_hip(const void* xrows, const void* xtp, const void* yrows, const void* ytp, const float* xyz, int R, int M,
                           float gamma, float* lse, float* soft, void* stream);
int gdm_soft_coord_bwd_hip(const void* xrows, const void* xtp, const void* yrows, const void* ytp, const float* xyz, int R, int M,
                           float gamma, const float* lse, const float* kb, float* gx, float* gy_part, float* gy, void* stream);
int gdm_soft_coord_bwd_parts(int R, int M);

/* ---------------------------------------------------------------------------------------
 * One attentive-pooling stage of RandLA-Net's local feature aggregation in a single launch (inference):
 * models/RandLA/RandLANet.py:700-718 Building_block.forward = two such stages; :720-727 relative_pos_encoding, :729-738
 * gather_neighbour, :747-754 Att_pooling.forward.  For every point i with neighbours idx[b,i,0..15]:
 *   f_xyz  = lrelu(s1 * (W1 . pos_enc(i, k)) + b1)                      (10 -> D/2; pos_enc = [dist, rel(3), tile(3), neighbour(3)])
 *   f_xyz  = lrelu(s2 * (W2 . f_xyz) + b2)                              only when w2t != NULL (the block's second stage, mlp2)
 *   f_cat  = [feat[:, idx[b,i,k]] ; f_xyz]                              (D x 16)
 *   att    = Wf . f_cat ; score = softmax_k(att) ; agg = sum_k f_cat * score
 *   out[b,:,i] = lrelu(sm * (Wm . agg) + bm)                            (D -> OUT <= D)
 * xyz f32[B,n,3], idx i32[B,n,16], feat f32[B,D/2,n], out f32[B,OUT,n]; weights TRANSPOSED ([in][out], contiguous):
 * w1t [10,D/2], w2t [D/2,D/2], wft [D,D], wmt [D,OUT]; s*, b* = eval-mode BatchNorm folded to scale / shift.  D in {32,64,128,256}. */
int gdm_lfa_stage_hip(const float* xyz, const int32_t* idx, const float* feat, const float* w1t, const float* s1, const float* b1,
                      const float* w2t, const float* s2, const float* b2, const float* wft, const float* wmt, const float* sm,
                      const float* bm, int B, int n, int K, int D, int OUT, float slope, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Pose solve statistics (evaluator.py:85-100 + utils/pvn3d_eval_utils_kpls.py:43-77 best_fit_transform).
 * Per crop, over the points with mask != 0: out[b] = { n, sum A (3), sum B (3), sum A_i B_j (9, row-major) } as f64,
 * A = model_xyz[best_idx] (f32[M,3]), B = scene point.  Scene xyz addressing: element (b, i, c) at
 * scene_xyz[b*scene_bstride + i*pt_stride + c*ch_stride] (so both [B,N,3] and the first rows of cld_rgb_nrm [B,9,N] work). */
int gdm_kabsch_stats_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* model_xyz,
                         const int32_t* best_idx, const uint8_t* mask, int B, int N, int M, double* out, void* stream);

/* The fit itself (pvn3d_eval_utils_kpls.py:55-77: centroids, SVD of H, reflection fix, t = cB - R cA) from those statistics,
 * on the device: RT f32[B,3,4] maps model coordinates (A) to the camera frame (B); valid u8[B] = n >= min_points, else the
 * reference's sentinel pose [I | (0,0,-1000)] (evaluator.py:94-96).  The optimal proper rotation is obtained as Horn's unit
 * quaternion (largest eigenvector of a symmetric 4x4, cyclic Jacobi, f64) -- the same R as SVD + reflection fix. */
int gdm_kabsch_solve_hip(const double* stats, int B, int min_points, float* RT, uint8_t* valid, void* stream);

/* The weighted fit.  gdm_kabsch_stats_w_hip: out[b] = { sum w, sum w A (3), sum w B (3), sum w A_i B_j (9) } as f64 over the points
 * with mask != 0 and a finite weight > 0 (weight f32[B,N]; NaN, infinite, zero and negative weights are skipped), count i32[B] = the
 * number of such points.  A = target[b, i] (f32[B,N,3], e.g. soft_xyz of gdm_match_soft_packed_hip) when target is non-NULL, else
 * model_xyz[best_idx] as gdm_kabsch_stats_hip (model_xyz / best_idx may then not be NULL; with a target they are ignored).
 * gdm_kabsch_solve_w_hip: the fit of gdm_kabsch_solve_hip with n = sum w (it is scale-free in n: weights c w give the pose of
 * weights w); valid = count >= min_points and sum w > 0, else the sentinel pose. */
int gdm_kabsch_stats_w_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* model_xyz,
                           const int32_t* best_idx, const float* target, const float* weight, const uint8_t* mask, int B, int N,
                           int M, double* out, int32_t* count, void* stream);
int gdm_kabsch_solve_w_hip(const double* stats, const int32_t* count, int B, int min_points, float* RT, uint8_t* valid, void* stream);

/* The differentiable pose-fit loss (opt-in, training; no counterpart in the reference): the mean model-point distance between the
 * weighted fit of soft targets and the ground-truth pose, with its gradient with respect to the targets and the weights -- the
 * ADD-style error the evaluator reports, seen by training.  Forward and backward are own kernels: no library SVD, no host read, a
 * fixed number of launches (two forward, one backward), so the step captures in a hipGraph.
 *
 * THE POSE LOSS RULE, per crop b.  Inputs: scene points B_i (f32, the addressing of gdm_kabsch_stats_hip; they carry no gradient),
 * targets A_i = target[b,i] (f32[B,N,3], model side), weights w_i = weight[b,i] (f32[B,N]), mask u8[B,N], the ground-truth pose
 * (Rg | tg) = RT_gt[b] (f32[B,3,4]), K model points X_k = model_pts (f32[K,3], shared by the crops; the first K rows of the model file,
 * a farthest-point subset by that file's contract) and S symmetry transforms (Rs | ts) = sym (f32[S,3,4], metres, shared; NULL = the
 * identity alone, S = 1).
 *   1. Statistics.  Exactly those of gdm_kabsch_stats_w_hip (that launch itself): the usable points (mask != 0 and a finite weight
 *      > 0), the skipped ones and the order of the sums are its own.  W = sum w, cA, cB, S = sum w (A - cA)(B - cB)^T.
 *   2. Fit.  The fp64 rotation R of the shared fragment (gdm_kabsch_fit.inc) before it is rounded, t = cB - R cA in fp64.  The f32 RT
 *      output is the fragment's own: gdm_kabsch_solve_w_hip's bit for bit.
 *   3. State, u8.  1 = too few: fewer than min_points usable points or W <= 0 (RT is the sentinel pose, as gdm_kabsch_solve_w_hip
 *      writes it), or a ground-truth pose that is not finite (RT is still the fit).  2 = ill-conditioned: with l1 >= l2 >= l3 the
 *      eigenvalues of P = (R S + (R S)^T) / 2, l2 + l3 <= cond_min l1 (the fit is not unique at l2 + l3 = 0: collinear points, or a
 *      plane whose mirror image fits as well).  0 = fitted.  A crop whose state is not 0 has loss 0, sym_idx -1 and every gradient 0.
 *   4. Loss.  e_sk = (R X_k + t) - (Rg (Rs X_k + ts) + tg) in fp64, D_s = (1/K) sum_k |e_sk| summed in one fixed order (lanes stride
 *      k, one butterfly per wave, waves left to right), loss = min_s D_s, the lowest s on a tie; sym_idx = that s.
 *   5. Pose gradient, over the winner only, e^ = e / |e| (0 where |e| = 0): G = dloss/dR = (1/K) sum_k e^_k X_k^T, g = dloss/dt =
 *      (1/K) sum_k e^_k.
 *   6. Fit adjoint.  G' = G - g cA^T, Z = G' R^T, Za = (Z - Z^T) / 2; the antisymmetric Omega with Omega P + P Omega = Za, i.e.
 *      (tr(P) I - P) omega = axial(Za), whose eigenvalues l_i + l_j state 2 keeps away from 0; Gamma = dloss/dS = -2 R^T Omega,
 *      dloss/dcA = -R^T g, dloss/dcB = g.
 *   7. Per usable point: dloss/dA_i = w_i [Gamma (B_i - cB) - R^T g / W],
 *      dloss/dw_i = (A_i - cA)^T Gamma (B_i - cB) - (A_i - cA) . R^T g / W + (B_i - cB) . g / W; both 0 for a skipped point; both
 *      times grad_loss[b], rounded once to f32.  No point's gradient is a sum over other points: no atomics, and eager, repeated and
 *      replayed runs give the same bits.
 * gdm_pose_loss_fwd_hip -> loss f64[B], RT f32[B,3,4], state u8[B], sym_idx i32[B] and the record: device memory aligned to 8 bytes of
 * at least gdm_pose_loss_record_bytes(B) bytes (the 16 statistics, GDM_POSE_LOSS_REC doubles and the usable-point count per crop), the
 * only workspace; it is what the backward reads instead of refitting.  gdm_pose_loss_bwd_hip: the same scene, target, weight and mask,
 * that record, grad_loss f64[B] -> grad_target f32[B,N,3], grad_weight f32[B,N], every element written.
 * 1 <= S <= GDM_POSE_LOSS_MAX_S, 0 <= cond_min < 1, B <= 65535; cond_min = 1e-3 is the default of a definition, not a tuned value. */
enum { GDM_POSE_LOSS_MAX_S = 64, GDM_POSE_LOSS_REC = 32 };
size_t gdm_pose_loss_record_bytes(int B);
int gdm_pose_loss_fwd_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* target,
                          const float* weight, const uint8_t* mask, const float* RT_gt, const float* model_pts, const float* sym, int B,
                          int N, int K, int S, int min_points, double cond_min, void* record, size_t record_bytes, double* loss,
                          float* RT, uint8_t* state, int32_t* sym_idx, void* stream);
int gdm_pose_loss_bwd_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* target,
                          const float* weight, const uint8_t* mask, const void* record, size_t record_bytes, const double* grad_loss,
                          int B, int N, float* grad_target, float* grad_weight, void* stream);

/* Robust fit: the reference's RANSAC (utils/pvn3d_eval_utils_kpls.py:79-124 best_fit_transform_with_RANSAC, used next to
 * best_fit_transform by evaluator.py:21) for a whole batch, every hypothesis evaluated at once.  Same correspondences as
 * gdm_kabsch_stats_hip (same arguments), plus `stats` = its output for them.  H = max_iter hypotheses per crop:
 *   h = 0      the Kabsch fit of all n selected pairs (what gdm_kabsch_solve_hip returns);
 *   h >= 1     the Kabsch fit of 4 pairs drawn with replacement from the selected pairs in point order (np.random.randint(0, n, 4)
 *              indexing A[cls_msk]; the reference's draw of iteration i is hypothesis i + 1, its last draw is never scored).
 *              Sampling is a stateless counter-based hash (no host RNG; eager, graph and forked-graph runs are bit-identical):
 *                mix(x) = lowbias32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *                r      = mix(mix(mix(seed ^ 0x9e3779b9) ^ b) ^ (4 h + s)),  s = 0..3
 *                index  = (uint64(r) * n) >> 32
 *              (restated in Python as pose.ransac_sample_indices).
 * counts i32[B,H]: c_h = #{selected pairs with |R a + t - b|^2 <= match_err^2}, fp32, integer counts (no float atomics).
 * Selection (the reference's sequential rule): the FIRST h with c_h > fix_percent * n (fp64) wins and RT is the Kabsch refit on its
 * inliers; otherwise the largest c_h wins (lowest h on ties) and RT is that hypothesis, without a refit.  winner i32[B] = that h.
 * n < min_points -> the sentinel [I | (0,0,-1000)], valid = 0, winner = -1.  Every c_h == 0 -> the same sentinel, valid = 0,
 * winner = -1 (the one deliberate deviation: the reference returns an all-zero matrix there).
 * 1 <= H <= GDM_RANSAC_MAX_H, match_err > 0, 0 < fix_percent <= 1, B <= 65535.  workspace: device memory, 16-byte aligned, of at
 * least gdm_ransac_workspace_bytes(B, N, H) bytes (the compacted pairs and the H hypothesis poses of every crop). */
#define GDM_RANSAC_MAX_H 4096
size_t gdm_ransac_workspace_bytes(int B, int N, int H);
int gdm_ransac_pose_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* model_xyz,
                        const int32_t* best_idx, const uint8_t* mask, const double* stats, int B, int N, int M, int H,
                        float match_err, double fix_percent, uint32_t seed, int min_points, void* workspace, size_t workspace_bytes,
                        float* RT, uint8_t* valid, int32_t* counts, int32_t* winner, void* stream);

/* Consensus fit from pairwise-compatible correspondences (no counterpart in the reference; the idea of spectral matching and of
 * SC^2-PCR's second-order spatial compatibility, parity with either is not claimed): two correct matches of a rigid object keep their
 * distance, so counting which pairs agree with which finds the consistent set without a draw.  Deterministic, a fixed set of
 * launches, no host synchronisation.  Same correspondences and scene addressing as gdm_kabsch_stats_hip.
 *
 * THE CONSENSUS RULE, per crop b.  The selected pairs are the points with mask != 0 in point order, compacted to k = 0..n-1; pair k
 * holds two fp32 points: the scene point p_k and the model point q_k = model_xyz[clamp(best_idx, 0, M-1)].
 *   1. Compatibility bit.  fp32 throughout, every product and sum rounded once (no contraction), no square root.  With d = p_i - p_j:
 *        a2 = ((dx dx) + dy dy) + dz dz,  b2 the same for q,  u = (a2 + b2) - tau tau  (tau tau one fp32 product),
 *        C_ij = (i != j) and (u <= 0 or u u <= (4 a2) b2)
 *      -- in real arithmetic | |p_i - p_j| - |q_i - q_j| | <= tau.  C is symmetric by construction.
 *   2. Degree and score, integers.  row_i = { j : C_ij },  deg_i = |row_i|,  s_i = sum_{j in row_i} |row_i & row_j|  (<= n^2, int32).
 *   3. Seeds, sequential, integers only.  covered = {}.  For t = 0..seeds-1: g_t = the uncovered pair with the largest s, the smallest
 *      k on a tie; when no uncovered pair has s > 0, this seed and every later one is -1.  Then covered gains row_g and g itself.
 *   4. Hypothesis t: a weighted least-squares fit.  Every j in row_g has w_j = |row_g & row_j|, the seed itself w_g = deg_g (exact
 *      integers); the 16 weighted statistics of gdm_kabsch_stats_w_hip over the pairs with w > 0, accumulated in fp64 in a fixed order,
 *      solved as gdm_kabsch_solve_w_hip solves them.  Fewer than 3 pairs with w > 0 (or no seed): the hypothesis is skipped, its
 *      count is -1 and its pose the sentinel.
 *   5. Count.  c_t = #{ selected pairs with |R_t q + t_t - p|^2 <= inlier_dist^2 }, the fp32 residual of gdm_ransac_pose_hip,
 *      integer counts (no float atomics).
 *   6. Winner.  The largest c_t wins, the smallest t on a tie, and RT is the unweighted Kabsch refit on its inliers (fp64 sums in a
 *      fixed order).  valid = n >= min_points and c_winner >= min_points; otherwise the sentinel [I | (0,0,-1000)], valid = 0,
 *      winner = -1.  Steps 1-5 do not look at min_points.
 * The final score is an inlier count, as RANSAC's is: a clump of wrong pairs collapsed onto one vertex and one scene spot that
 * outnumbers the true inliers wins.  Judging candidates by the depth frame is gdm_pose_verify_hip's part.
 * Outputs: RT f32[B,3,4], valid u8[B], score / degree i32[B,N] (s and deg per POINT, -1 where mask == 0), seed_idx i32[B,seeds]
 * (point indices, -1 = unused), hyp_RT f32[B,seeds,3,4], counts i32[B,seeds], winner i32[B] (the t that won).
 * 1 <= N <= 4096 (a bit row is held one 64-bit word per lane), 1 <= seeds <= 64, tau > 0, inlier_dist > 0, min_points >= 3,
 * B <= 65535.  workspace: device memory aligned for uint64_t, of at least gdm_consensus_workspace_bytes(B, N, seeds) bytes (0 for
 * shapes beyond these limits): the compacted pairs, per-pair integers and an n x n BIT matrix per crop, ceil(N/64) words a row --
 * 512 KiB per crop at N = 2048, 2 MiB at 4096.  No n x n float tensor is formed. */
size_t gdm_consensus_workspace_bytes(int B, int N, int seeds);
int gdm_consensus_pose_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* model_xyz,
                           const int32_t* best_idx, const uint8_t* mask, int B, int N, int M, int seeds, float tau, float inlier_dist,
                           int min_points, void* workspace, size_t workspace_bytes, float* RT, uint8_t* valid, int32_t* score,
                           int32_t* degree, int32_t* seed_idx, float* hyp_RT, int32_t* counts, int32_t* winner, void* stream);

/* Point-to-point ICP refinement, scene -> model (utils/pvn3d_eval_utils_kpls.py:126-212 icp, run as icp(scene, model, RT^-1)).
 * One iteration = gdm_icp_transform_hip, an exact K = 1 search of the query among the model vertices (gdm_knn_jobs_ws_hip, support
 * batch stride 0, with d2), gdm_icp_update_hip.
 * gdm_icp_transform_hip: query f32[B,N,3] = R^T (b - t) for every scene point b (same addressing as gdm_kabsch_stats_hip), RT f32[B,3,4].
 * gdm_icp_update_hip: for every crop with active != 0, the pairs (model_xyz[nn], b) of the points with mask != 0 (and, when
 * reject_dist >= 0, d2 <= reject_dist^2) -> fp64 statistics -> RT is refit (absolute pose), iters += 1, mean = mean pair distance
 * (before the update, as :193-204); |err - mean| < tolerance sets active = 0; err = mean.  err starts at 0 (prev_error = 0, :189).
 * Fewer than min_points pairs: active = 0 and the crop is left unchanged.  nn i32[B,N], d2 f32[B,N] (the K = 1 search),
 * active u8[B], iters i32[B], err f64[B] are read and written: a fixed number of iterations runs without host synchronisation. */
int gdm_icp_transform_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* RT, int B, int N,
                          float* query, void* stream);
int gdm_icp_update_hip(const float* scene_xyz, long scene_bstride, int pt_stride, int ch_stride, const float* model_xyz,
                       const int32_t* nn, const float* d2, const uint8_t* mask, int B, int N, int M, float reject_dist,
                       double tolerance, int min_points, float* RT, uint8_t* active, int32_t* iters, double* err, void* stream);

/* Point-to-plane ICP refinement, scene -> model (opt-in; no counterpart in the reference).  One iteration = gdm_icp_transform_hip,
 * the same K = 1 search, gdm_icp_plane_update_hip: one Gauss-Newton step per crop on the point-to-plane residual, in the model frame.
 * For a crop with active != 0 and pose (R, t) = RT[b] (fp32, widened to fp64):
 *   Pairs.  For every point i with mask != 0: x = query[b,i] (the fp32 row gdm_icp_transform_hip wrote), j = clamp(nn[b,i], 0, M-1),
 *     q = model_xyz[j], n = model_nrm[j] (f32[M,3], used as given: the caller supplies unit normals).  The pair is dropped when
 *     reject_dist >= 0 and max(d2[b,i], 0) > reject_dist^2 (fp32, as gdm_icp_update_hip), or when scene_nrm != NULL and
 *     (R^T s_i) . n < normal_gate (fp64; s_i = the scene normal of point i, element (b, i, c) at
 *     scene_nrm[b*scene_bstride + i*pt_stride + c*ch_stride] -- rows 6..8 of cld_rgb_nrm; -1 <= normal_gate <= 1).
 *     scene_nrm == NULL turns the gate off (the strides and normal_gate are then ignored).
 *   Sums (fp64, fixed reduction order, no atomics).  r = n . (x - q); w = 1 when huber_delta <= 0 or |r| <= huber_delta, else
 *     huber_delta / |r|; J = [x cross n ; n];  A = sum w J J^T, g = sum w J r, S = sum w, L2 = sum w |x|^2, E = sum |r|, n_pairs.
 *   Starved.  n_pairs < max(min_points, 6): active = 0, status = 2, the crop is left unchanged.
 *   Degenerate (unit-free).  l2 = L2 / S, D = diag(1/sqrt(l2) x3, 1 x3), A^ = D A D / S factored by Cholesky in that order without
 *     pivoting; l2 <= 0 or a pivot L_kk^2 < pivot_min (> 0; 1e-6 is the package default): active = 0, status = 3, the crop is left
 *     unchanged (a plane patch, a sphere about the origin, a body of revolution about an axis through it).
 *   Update.  A xi = -g through that factor, xi = (omega, v); R_inc = exp([omega]x) by Rodrigues (I + [omega]x below |omega| = 1e-8);
 *     R <- R R_inc^T, t <- t - R_new v, both stored as fp32.
 *   Stop (as gdm_icp_update_hip).  iters += 1, mean = E / n_pairs; |err - mean| < tolerance sets active = 0 and status = 1; err = mean.
 * status i32[B] is written only on those three events (start it at 0: 0 = still running or never run); active u8[B], iters i32[B],
 * err f64[B] are read and written, so a fixed number of iterations runs without host synchronisation.  n_pairs i32[B] (may be
 * NULL): the pairs kept in this call, written for every crop that was active on entry. */
int gdm_icp_plane_update_hip(const float* scene_nrm, long scene_bstride, int pt_stride, int ch_stride, const float* query,
                             const float* model_xyz, const float* model_nrm, const int32_t* nn, const float* d2, const uint8_t* mask,
                             int B, int N, int M, float reject_dist, double normal_gate, double huber_delta, double tolerance,
                             int min_points, double pivot_min, float* RT, uint8_t* active, int32_t* iters, double* err,
                             int32_t* status, int32_t* n_pairs, void* stream);

/* Ground-truth correspondence targets: the reference loader's get_pose_gt_info (datasets/lm/linemod_pbr.py:602-655) for a batch.
 * workspace: device memory, 16-byte aligned, of at least gdm_targets_workspace_bytes(B, N, M) bytes (any N >= 1 for
 * gdm_hpr_visible_hip alone); 0 for a bad shape.  M >= GDM_TARGETS_MIN_M, B <= 65535.
 * Model addressing: vertex (b, j) at model_xyz[b*model_bstride + 3*j] (f32 xyz, metres); model_bstride = 0 shares one cloud.
 *
 * gdm_hpr_visible_hip -- hidden-point removal (utils/compute_visibility.py:26-47 sphericalFlip / convexHull, :128-134 VisiblePoints):
 *   camera centre c f32[3]: cam_center[b] when cam_center != NULL, else fp32(-R^T t) evaluated in fp64 as
 *     c_k = -((R_0k t_0 + R_1k t_1) + R_2k t_2)
 *     (a deviation: the reference inverts the fp32 4x4 [R t; 0 1] with LAPACK, :617-623, whose rounding can differ by an ulp);
 *   p = v - c (fp32), n = sqrt((p_x^2 + p_y^2) + p_z^2) (fp32), Rad = fp64(max_j n_j) * 10^pi (10^pi = 1385.4557313670107),
 *   flipped f64[B,M,3] = (2 ((Rad - n) p)) / n + p in fp64 -- bit-equal to sphericalFlip for the same centre.
 *   visible u8[B,M] = 1 for the hull vertices of {f} U {origin}, then the reference's vertices[:-1]: when the origin is not a vertex
 *   of that hull the highest-index visible vertex is dropped as well.  Vertex test: f_i is a vertex iff no point of the set lies
 *   in conv(the others), decided per (crop, vertex) as a 2-D LP feasibility problem in fp64 (directions d = f_i/|f_i| + a e1 + b e2,
 *   |a|, |b| <= 1e6) with Seidel's incremental algorithm in a fixed hashed order; exact for points in general position (no four
 *   coplanar hull points through f_i), which is where Qhull's answer is defined.  Among exactly coincident flipped points only the
 *   lowest index can be visible.  The camera centre must not coincide with a vertex (n = 0).
 *
 * gdm_pose_targets_hip -- the targets from that visibility (:632-655):
 *   the visible vertices are posed in fp32 as ((r_0 x + r_1 y) + r_2 z) + t; for every point with labels != 0 (cld addressing as
 *   gdm_kabsch_stats_hip) the nearest posed visible vertex by fp64 ((dx^2 + dy^2) + dz^2) from the fp32 coordinates, ties to the
 *   lowest model index (sklearn NearestNeighbors, utils/icp.py:50-64); sqrt(d^2) > dist_thresh -> match M and label 0.
 *   labels_out u8[B,N] (may alias labels), match_idx i32[B,N] (M where unmatched or unlabelled), visible_flag u8[B,M], valid u8[B]:
 *     no labelled point             -> labels unchanged, match_idx all M, visible_flag all 0, valid 0 (:626-630);
 *     every labelled point too far  -> labels unchanged, match_idx all M, visible_flag = visible, valid 0 (:644-646);
 *     otherwise                     -> as above, valid 1. */
#define GDM_TARGETS_MIN_M 4
size_t gdm_targets_workspace_bytes(int B, int N, int M);
int gdm_hpr_visible_hip(const float* model_xyz, long model_bstride, const float* RT, const float* cam_center, int B, int M,
                        void* workspace, size_t workspace_bytes, double* flipped, uint8_t* visible, void* stream);
int gdm_pose_targets_hip(const float* cld, long cld_bstride, int pt_stride, int ch_stride, const uint8_t* labels, const float* RT,
                         const float* model_xyz, long model_bstride, const uint8_t* visible, int B, int N, int M, double dist_thresh,
                         void* workspace, size_t workspace_bytes, uint8_t* labels_out, int32_t* match_idx, uint8_t* visible_flag,
                         uint8_t* valid, void* stream);

/* Eval-mode BatchNorm + activation + max over the K neighbours (DGCNN edge convolutions, dgcnn.py:104-117) in one pass:
 * out[plane,i] = max_k act(scale[c]*x[plane,i,k] + shift[c]), c = plane % C; x f32[planes,n,K], K % 4 == 0, planes <= 65535. */
int gdm_affine_act_maxk_hip(const float* x, const float* scale, const float* shift, long planes, int C, long n, int K, int act,
                            float slope, float* out, void* stream);

/* Single-slope PReLU (models/cnn/pspnet.py:41) and its backward, for training: y = x > 0 ? x : a x; grad_x = x > 0 ? go : a go;
 * grad_slope[0] += sum over x <= 0 of x * go (zeroed by the caller).  slope is a DEVICE pointer to the one parameter; n % 4 == 0. */
int gdm_prelu1_hip(const float* x, const float* slope, long n, float* y, void* stream);
int gdm_prelu1_bwd_hip(const float* x, const float* grad_out, const float* slope, long n, float* grad_x, float* grad_slope, void* stream);

/* Inference-mode BatchNorm + activation (+ residual branch with its own folded BatchNorm) in one pass:
 * y = act(x*scale[c] + shift[c] (+ res*res_scale[c] + res_shift[c])), c = plane % C; x,res,y f32[planes, inner],
 * inner % 4 == 0; res / res_scale / res_shift may be NULL (res_scale NULL = plain residual add).
 * act: 0 none, 1 ReLU, 2 leaky ReLU / single-slope PReLU (slope).  May run in place (y == x).
 * Replaces the BN / ReLU / LeakyReLU / PReLU / add launches of pytorch_utils._ConvBase, extractors.BasicBlock
 * (extractors.py:36-58), PSPUpsample (pspnet.py:34-45) and Dilated_res_block (RandLANet.py:683-688) in eval mode. */
int gdm_affine_act_hip(const float* x, const float* scale, const float* shift, const float* res, const float* res_scale,
                       const float* res_shift, long planes, int C, long inner, int act, float slope, float* y, void* stream);

/* conv3x3(pad 1) after bilinear upsample (align_corners), from low-resolution channel mixes (pspnet.py:34-45):
 * z f32[B, 9*Cout, H, W] = conv1x1(x, W rearranged tap-major) at LOW resolution; this gathers, per output pixel,
 * the 9 bilinear taps (zero outside the OHxOW map), applies scale/shift (folded BN incl. the conv bias) and the
 * activation (0 none, 1 ReLU, 2 leaky/PReLU slope) -> out f32[B, Cout, OH, OW].                              */
int gdm_upconv3x3_gather_hip(const float* z, const float* scale, const float* shift, int B, int Cout, int H, int W,
                             int OH, int OW, int act, float slope, float* out, void* stream);
/* The same with eight output channels per workgroup, also writing the result as the packed split-bf16 operand (gdm_conv3x3_act_bytes
 * (B, Cout, OH, OW) bytes, zero border kept by the caller) of the next GEMM over the map: Cout = 64 or a multiple of 128, x2 stages. */
int gdm_upconv3x3_gather2_hip(const float* z, const float* scale, const float* shift, int B, int Cout, int H, int W,
                              int OH, int OW, int act, float slope, float* out, void* outpk, void* stream);
/* Its transpose for training (scale = 1, act = none): grad_z f32[B,9*Cout,H,W] from grad_out f32[B,Cout,OH,OW]; every element of
 * grad_z is written (gather form, no atomics).  B*9*Cout <= 65535. */
int gdm_upconv3x3_gather_bwd_hip(const float* grad_out, int B, int Cout, int H, int W, int OH, int OW, float* grad_z, void* stream);
/* The whole PSPUpsample(64 -> 64) in one kernel (the last up stage, where the 9*64-channel low-resolution tensor of the two-kernel
 * form is 604 MB at batch 16): x f32[B,64,H,W] -> out f32[B,64,OH,OW] = act(scale * conv3x3(upsample(x)) + shift), weights packed by
 * gdm_upconv_fused64_pack_weight_hip from the f32[64,64,3,3] convolution weight (split-bf16 products, fp32 accumulate). */
size_t gdm_upconv_fused64_weight_bytes(void);
int gdm_upconv_fused64_pack_weight_hip(const float* w, void* wpk, void* stream);
int gdm_upconv_fused64_hip(const float* x, const void* wpk, const float* scale, const float* shift, int B, int C, int H, int W,
                           int OH, int OW, int act, float slope, float* out, void* stream);

/* Pyramid-pooling bottleneck tail (pspnet.py:24-31) after splitting the 1x1 convolution over the concat:
 * out = relu(g + bias[c] + sum_k bilinear_align_corners(y_k)), g f32[B,C,H,W] = W_f . feats, y_k f32[B,C,s_k,s_k] = W_k . prior_k.
 * outpk (may be NULL): the result also as the packed split-bf16 operand (gdm_conv3x3_pack_act_hip's layout, gdm_conv3x3_act_bytes
 * bytes, zero border kept by the caller) of the next GEMM over the map: C = 64 or a multiple of 128, W % 4 == 0. */
int gdm_psp_combine2_hip(const float* g, const float* y1, int s1, const float* y2, int s2, const float* y3, int s3,
                         const float* y4, int s4, const float* bias, int B, int C, int H, int W, float* out, void* outpk, void* stream);
/* Point->pixel fusion tail (ffb6d.py:216-222,252-258): y[b,c,j] = act(scale[c]*(x[b,c,j] + t[b,c,idx[b,j]]) + shift[c]),
 * x f32[B,C,m] (pixel half of the 1x1 conv), t f32[B,C,n] (point half, computed at the points), idx i32[B,m]. May run in place.
 * With y_packed != NULL the result is ALSO written as the packed split-bf16 operand of the next convolution / GEMM over the
 * [B, C, m/W, W] map (gdm_conv3x3_act_bytes(B, C, m/W, W) bytes, zero border in place; C = 64 or a multiple of 128): no pack launch
 * in front of that layer.  W is read only with y_packed.  y may be NULL when y_packed is given: the packed operand is then the only
 * output (no fp32 store, x is left untouched), for a map whose only reader is a GEMM on the packed operand. */
int gdm_gather_add_affine_act2_hip(const float* x, const float* t, const int32_t* idx, const float* scale, const float* shift,
                                   int B, int C, int n, int m, int act, float slope, float* y, void* y_packed, int W, void* stream);
/* The same tail with the pixel half of the 1x1 convolution inside, for the 64-channel levels (C == 64):
 * y[b,co,j] = act(scale[co]*(sum_ci W[co,ci] x[b,ci,j] + t[b,co,idx[b,j]]) + shift[co]); wt f32[C,C] = W transposed ([ci][co]).
 * pixel_major = 0 writes y f32[B, C, m]; != 0 writes y f32[B, m, C] (one 256-byte row per pixel, y 16-byte aligned). */
int gdm_conv1x1_gather_add_act2_hip(const float* x, const float* wt, const float* t, const int32_t* idx, const float* scale,
                                    const float* shift, int B, int C, int n, long m, int act, float slope, int pixel_major,
                                    float* y, void* stream);
/* The same fusion with the K = 64 channel mix on the matrix cores (split-bf16 x3, fp32 accumulate): wpk = the 64 x 64 weight (row =
 * output channel) packed by gdm_pack_rows64_hip; t_point_major != 0: t is f32[B, n, 64] (the gathered term is then one contiguous
 * 256-byte row per pixel instead of 64 scattered floats); pixel_major and the other arguments as above.  With ypk != NULL (NCHW form
 * only) the result is ALSO written as the packed split-bf16 operand of the next convolution over the [B, 64, m / W, W] map
 * (gdm_conv3x3_act_bytes(B, 64, m / W, W) bytes, zero border kept by the caller).  W is read only with ypk.  A point-major t, a
 * pixel-major y and ypk must be 16-byte aligned (GDM_EINVAL otherwise). */
int gdm_conv64_gather_add_act_mfma2_hip(const float* x, const void* wpk, const float* t, const int32_t* idx, const float* scale,
                                        const float* shift, int B, int n, long m, int act, float slope, int pixel_major,
                                        int t_point_major, float* y, void* ypk, int W, void* stream);
/* That fusion (NCHW form, point-major t f32[B, n, 64]) and the `final` stage behind it in one launch, for a fused map only `final`
 * reads: out f32[B, 64, m] = log_softmax_c(Wf . y + fbias) with y the map gdm_conv64_gather_add_act_mfma2_hip would write; the same
 * bits as that call followed by gdm_conv1x1_logsoftmax_hip, without the map between them.  wft f32[64, 64] = the `final` weight
 * transposed ([ci][co]), fbias f32[64] or NULL.  t must be 16-byte aligned. */
int gdm_conv64_gather_add_final_hip(const float* x, const void* wpk, const float* t, const int32_t* idx, const float* scale,
                                    const float* shift, int B, int n, long m, int act, float slope, const float* wft,
                                    const float* fbias, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * 3x3 / stride 1 / pad 1 convolution as an implicit GEMM on split-bf16 MFMA (hi*hi + hi*lo + lo*hi, fp32 accumulate),
 * for the 32x32-resolution ResNet-18 layers (models/cnn/extractors.py:36-58,151-177) where MIOpen's fp32 path is a
 * vector-ALU Winograd kernel.  Cin, Cout multiples of 128, W a multiple of 32.
 *   pack_weight: w f32[Cout,Cin,3,3] -> wpk (gdm_conv3x3_weight_bytes), once per weight change
 *   pack_act   : x f32[B,Cin,H,W]    -> xpk (gdm_conv3x3_act_bytes; pixel-major rows with a one-pixel ZERO border: the
 *                caller provides a zero-filled buffer, only interior rows are written)
 *   packed     : out f32[B,Cout,H,W] = act(scale[co] * conv + shift[co] (+ res)), act 0 none / 1 ReLU; scale/shift/res may be NULL
 * THE OPERAND LIMIT of every entry point that launches this kernel -- gdm_conv3x3_packed_hip, gdm_conv3x3_strided_hip,
 * gdm_conv1x1_packed_hip, gdm_conv1x1_strided_hip, gdm_conv1x1_gather_add_hip, gdm_gemm_grouped_hip, gdm_conv1x1_packed_wb_hip: the kernel
 * addresses xpk and wpk with 32-bit byte offsets, so each must stay below 2 GiB (2^31 bytes).  xpk counts as the packed INPUT map,
 * gdm_conv3x3_act_bytes(B, Cin, H*stride, W*stride); wpk as gdm_conv3x3_weight_bytes / gdm_conv1x1_weight_bytes, behind (B - 1) *
 * w_bstride bytes where every image has its own weights.  A call past the limit is refused on the host before any HIP call (nonzero,
 * gdm_last_error() names the entry point and both byte counts); nothing is launched. */
size_t gdm_conv3x3_act_bytes(int B, int Cin, int H, int W);
size_t gdm_conv3x3_weight_bytes(int Cout, int Cin);
int gdm_conv3x3_pack_weight_hip(const float* w, int Cout, int Cin, void* wpk, void* stream);
int gdm_conv3x3_pack_act_hip(const float* x, int B, int Cin, int H, int W, void* xpk, void* stream);
/* Every convolution / GEMM entry below refuses (GDM_EINVAL) packed operands, a residual or an output off a 16-byte boundary. */
int gdm_conv3x3_packed_hip(const void* xpk, const void* wpk, const float* scale, const float* shift, const float* res,
                           int B, int Cin, int Cout, int H, int W, int act, float* out, void* stream);
/* Strided forms (stride 1 or 2; the first block of ResNet-18 layer2, extractors.py:151-177): H, W are the OUTPUT size, xpk is the
 * (H*stride) x (W*stride) input packed by gdm_conv3x3_pack_act_hip; gdm_conv1x1_strided_hip is the block's 1x1 downsample branch
 * on the same packed input (NCHW output).  gdm_conv3x3_strided_hip writes its result to out, to outpk as the packed operand of the
 * next convolution (gdm_conv3x3_act_bytes(B, Cout, H, W) bytes, zero-filled once by the caller; Cout % 8 == 0, B*H*W % 256 == 0),
 * which then needs no pack launch, or to both; either may be NULL, not both. */
int gdm_conv3x3_strided_hip(const void* xpk, const void* wpk, const float* scale, const float* shift, const float* res,
                            int B, int Cin, int Cout, int H, int W, int stride, int act, float* out, void* outpk, void* stream);
int gdm_conv1x1_strided_hip(const void* xpk, const void* wpk, const float* scale, const float* shift,
                            int B, int Cin, int Cout, int H, int W, int stride, int act, float* out, void* stream);
/* The point-to-pixel fusion in one launch: gdm_conv1x1_strided_hip (stride 1, no scale / shift) followed by
 * gdm_gather_add_affine_act2_hip, bit for bit, with the gather, the folded BatchNorm and the activation in the GEMM's epilogue:
 * out[b,co,j] = act(scale[co] * (sum_ci W[co,ci] x[b,ci,j] + gt[b,co,clamp(gidx[b,j], 0, gn-1)]) + shift[co]).
 * gidx int32[B,H*W] (16-byte aligned), gt f32[B,Cout,gn], gn >= 1; Cin a multiple of 128; act 0 (none) or 1 (ReLU).  out f32[B,Cout,H,W]
 * and / or outpk (the packed operand of the next convolution, as gdm_conv3x3_strided_hip writes it: Cout % 8 == 0, B*H*W % 256 == 0);
 * either may be NULL, not both.  The packed activations and the packed weights must each stay below 2 GiB (the operand limit above). */
int gdm_conv1x1_gather_add_hip(const void* xpk, const void* wpk, const int32_t* gidx, const float* gt, int gn, const float* scale,
                               const float* shift, int B, int Cin, int Cout, int H, int W, int act, float* out, void* outpk, void* stream);

/* `final` stage of the image branch (pspnet.py:108-112): out = log_softmax_c(W x + b), x,out f32[B,64,hw], W f32[64,64]. */
/* ResNet stem tail in one pass (extractors.py:128-131 after conv1): y = MaxPool2d(3, stride 2, padding 1)(relu(scale[c] * x + shift[c])),
 * x f32[B,C,H,W] -> y f32[B,C,(H-1)/2+1,(W-1)/2+1]; scale / shift = eval-mode BatchNorm folded. */
int gdm_affine_relu_maxpool_hip(const float* x, const float* scale, const float* shift, int B, int C, int H, int W, float* y, void* stream);
int gdm_conv1x1_logsoftmax_hip(const float* x, const float* w, const float* bias, int B, int C, long hw, float* out, void* stream);
/* The last image stage of FFB6DEmb at the SAMPLED pixels only (inference; /root/reference/models/ffb6d.py:266-285: cnn_up_stages[3] =
 * PSPUpsample(64 -> 64) + `final`, then torch.gather with `choose`): out f32[B,64,N] = log_softmax(Wf . act(scale * conv3x3(up(x)) +
 * shift) + fbias) at pixel choose[b,n] of the OHxOW map.  xpm f32[B, H*W, 64] is the source map PIXEL-major (written by
 * gdm_conv1x1_gather_add_act2_hip(pixel_major = 1)); wpk = gdm_upconv_fused64_pack_weight_hip's rows; wfpk = the 64x64 `final` weight
 * packed by gdm_pack_rows64_hip (R rows of 64 floats -> 256-byte split-bf16 rows); fbias may be NULL.  choose is clamped to the map. */
int gdm_pack_rows64_hip(const float* w, int R, void* out, void* stream);
int gdm_upconv_final_points_hip(const float* xpm, const int32_t* choose, const void* wpk, const float* scale, const float* shift,
                                int act, float slope, const void* wfpk, const float* fbias, int B, int H, int W, int OH, int OW,
                                int N, float* out, void* stream);
/* The four adaptive average pools (1,2,3,6 bins) of the pyramid pooling module (pspnet.py:17-20) in one pass:
 * x f32[planes,H,W] -> o1 f32[planes,1], o2 [planes,4], o3 [planes,9], o6 [planes,36] (PyTorch bin edges). */
int gdm_psp_pools_hip(const float* x, long planes, int H, int W, float* o1, float* o2, float* o3, float* o6, void* stream);
/* Its backward (training): grad_x[planes,H,W] = sum over every bin containing the pixel of grad_bin / bin area, all four sizes in one
 * pass (replaces four adaptive_avg_pool2d backward launches of `PSPModule.stages`, pspnet.py:17-20, and the sums that merge them). */
int gdm_psp_pools_bwd_hip(const float* g1, const float* g2, const float* g3, const float* g6, long planes, int H, int W,
                          float* grad_x, void* stream);

/* 1x1 convolution / GEMM on the same split-bf16 MFMA kernel (one tap): x packed by gdm_conv3x3_pack_act_hip, weights
 * f32[Cout,Cin] packed by gdm_conv1x1_pack_weight_hip.  out = act(scale*(W x)+shift) as f32[B,Cout,H,W], or, with
 * pixel_major != 0, as f32[B*H*W, Cout] (used for the dense part of SplineConv: nodes x (125*128)).  Cin % 128 == 0; Cout is
 * arbitrary: the packed weights carry zero rows up to the next multiple of 128 and the extra outputs are never stored.  The operand
 * limit above holds: a [B, Cin, n] product packed as a map of one row per image has B * 3 * (n + 2) * ceil(Cin / 128) * 512 bytes. */
size_t gdm_conv1x1_weight_bytes(int Cout, int Cin);
int gdm_conv1x1_pack_weight_hip(const float* w, int Cout, int Cin, void* wpk, void* stream);
/* training: the packed weights of the INPUT-GRADIENT convolution (the flipped, transposed filter) straight from the forward weight
 * w f32[Cout,Cin,taps], taps 9 (3x3/s1/p1) or 1: a layer with Cin outputs and Cout inputs (Cout % 128 == 0 or Cout == 64); wpk holds
 * gdm_conv3x3_weight_bytes(Cin, Cout) / gdm_conv1x1_weight_bytes(Cin, Cout) bytes.  Replaces the flip / transpose / contiguous copies
 * torch's convolution backward makes of the weights of models/cnn/extractors.py:36-58. */
int gdm_conv_pack_weight_dgrad_hip(const float* w, int Cout, int Cin, int taps, void* wpk, void* stream);
int gdm_conv1x1_packed_hip(const void* xpk, const void* wpk, const float* scale, const float* shift,
                           int B, int Cin, int Cout, int H, int W, int act, int pixel_major, float* out, void* stream);

/* Front end: depth (m) f32[B,H,W] + intrinsics K f32[B,3,3] + integer crop origin (x0,y0) i32[B,2] -> camera-frame
 * xyz f32[B,S,S,3] of the SxS crop (datasets/lm/linemod_pbr.py:398-411 dpt_2_pcld; zeros where depth <= 1e-8). */
int gdm_depth_to_xyz_hip(const float* depth, const float* K, const int32_t* origin, int B, int H, int W, int S,
                         float* out, void* stream);

/* Front end, surface normals from the depth image (the loader's normalSpeed.depth_normal(dpt_mm, fx, fy, 5, 2000, 20, False),
 * datasets/lm/linemod_pbr.py:460-463): depth (m) f32[B,H,W], K f32[B,3,3] -> normals f32[B,3,H,W], unit or zero, towards the camera
 * (nz <= 0).  The LINEMOD least-squares depth gradient, defined here operation by operation:
 *   d = (uint16) trunc(fp32(depth) * 1000.0f)   (negative and NaN -> 0; 65.535 m and beyond -> 65535)
 *   r = k_size; pixels with x < r, x >= W-r, y < r or y >= H-r -> (0,0,0);  c = d[y,x]; !(c < distance_threshold) -> (0,0,0)
 *   over the 8 offsets (i,j) in {-r,0,r}^2 \ (0,0), in integers:  delta = d[y+j,x+i] - c;  f = |delta| < difference_threshold;
 *     A0 += f i i; A1 += f i j; A3 += f j j; b0 += f i delta; b1 += f j delta
 *   det = A0 A3 - A1 A1; ddx = A3 b0 - A1 b1; ddy = -A1 b0 + A0 b1   (64-bit)
 *   nx = fp32(fx) * fp32(ddx); ny = fp32(fy) * fp32(ddy); nz = fp32(-(det c));  fx = K[0][0], fy = K[1][1]
 *   s = sqrtf((nx nx + ny ny) + nz nz);  s > 0 ? (nx/s, ny/s, nz/s) : (0,0,0)   (fp32, no contraction)
 * 1 <= k_size <= GDM_NORMALS_MAX_K and both thresholds in [0, 65536], which keeps every integer above inside its type. */
#define GDM_NORMALS_MAX_K 64
int gdm_depth_normals_hip(const float* depth, const float* K, int B, int H, int W, int k_size, int distance_threshold,
                          int difference_threshold, float* normals, void* stream);

/* Front end, the resampling crop around a detection box (the loader's six crop_resize_by_warp_affine calls, linemod_pbr.py:468-473):
 * rgb u8[B,H,W,3], depth f32[B,H,W], normals f32[B,3,H,W], K f32[B,3,3], mask u8[B,H,W] or NULL, center f32[B,2] = (cx,cy) and
 * scale f32[B] in source pixels -> out_rgb f32[B,3,S,S] (bilinear on uint8, then normalize_color: / 255, - mean, / std with std
 * .229/.224/.224), out_normals f32[B,3,S,S] (bilinear), out_xyz f32[B,S,S,3] (dpt_2_pcld of the nearest source pixel, the arithmetic
 * of gdm_depth_to_xyz_hip), out_depth f32[B,S,S] and out_mask u8[B,S,S] (nearest; out_mask NULL exactly when mask is).  normals and
 * out_normals may both be NULL: no normals are cropped (the YCB-V item computes them on the filled crop instead).
 * OpenCV's fixed-point warpAffine with BORDER_CONSTANT 0 for a pure scale + shift:
 *   a = fp64(scale)/S; bx = fp64(cx) - (a S)/2; by = fp64(cy) - (a S)/2;  R(v) = round-half-even(v * 1024) as an integer
 *   nearest: X = (R(a x) + R(bx) + 512) >> 10;  Y = (R(a y + by) + 512) >> 10
 *   linear:  X5 = (R(a x) + R(bx) + 16) >> 5;  Y5 = (R(a y + by) + 16) >> 5;  sx = X5 >> 5, al = X5 & 31;  sy = Y5 >> 5, be = Y5 & 31
 *            taps (sy,sx) (sy,sx+1) (sy+1,sx) (sy+1,sx+1); a tap outside the frame contributes 0
 *     uint8: w = 32 {(32-be)(32-al), (32-be) al, be (32-al), be al};  out = (sum w_k v_k + 16384) >> 15
 *     float: w = {(1-be/32)(1-al/32), (1-be/32)(al/32), (be/32)(1-al/32), (be/32)(al/32)} in fp32;
 *            out = ((v0 w0 + v1 w1) + v2 w2) + v3 w3   (fp32, no contraction)
 * With scale == S and center = (x0 + S/2, y0 + S/2) this is the integer crop at (x0, y0). */
int gdm_warp_crop_hip(const uint8_t* rgb, const float* depth, const float* normals, const float* K, const uint8_t* mask,
                      const float* center, const float* scale, int B, int H, int W, int S, float* out_rgb, float* out_normals,
                      float* out_xyz, float* out_depth, uint8_t* out_mask, void* stream);

/* Front end, depth completion of a cropped depth image (the YCB-V loader's `fill_missing(dpt, 1, 1)`, datasets/ycbv/ycbv_pbr.py:477:
 * IP-Basic's fill_in_multiscale, or fill_in_fast, with their defaults, utils/ip_basic/depth_map_utils.py): depth (m) f32[B,H,W] ->
 * out f32[B,H,W].  Defined here operation by operation, in fp32, from the documented meaning of the cv2 calls the reference makes
 * (equality with a given cv2 build is unpinned):
 *   in = depth > 0 ? depth : 0   (negative and NaN -> 0);  the thresholds are fp32(0.1), fp32(15), fp32(30)
 *   inv(d) = d > 0.1 ? max_depth - d : d   (one fp32 subtraction)
 *   dilate(a, k)[y,x] = max of a[y+dy,x+dx] over the nonzero (dy,dx) of k, anchored at its centre, taps outside the image ignored;
 *     erode = min under the same rule;  close(a, k) = erode(dilate(a, k), k)
 *     FULL_n: all of n x n;  CROSS_n: the centre row and the centre column of n x n;  DIAMOND_5: |dy| + |dx| <= 2
 *   median5(a)[y,x] = the 13th smallest of the 5 x 5 window, coordinates clamped to the image (replicated border)
 *   bilateral(a, sc, ss)[y,x]: the 13 taps with dx^2 + dy^2 <= 4 in row-major order (dy outer, from -2), coordinates reflected
 *     (-1 -> 1, n -> n-2) and then clamped to the image;  cc = fp32(-0.5 / (sc sc)), ws(r2) = fp32(exp(-0.5 r2 / (ss ss))) (fp64 inside);
 *     per tap v:  dv = v - a[y,x];  e = (dv dv) cc;  w = ws(dx^2+dy^2) expf(e);  num = num + w v;  den = den + w;   out = num / den
 *     (no contraction; cv2 interpolates a table whose range depends on the image -- the formula is defined, not the table)
 * mode GDM_FILL_MULTISCALE (extrapolate=False, blur_type='bilateral'):
 *   near = 0.1 < in <= 15; med = 15 < in <= 30; far = in > 30;   s1 = inv(in)
 *   s2 = s1, then overwritten where D > 0.1 by D = dilate(far ? s1 : 0, CROSS_3), then by dilate(med ? s1 : 0, CROSS_5), then by
 *     dilate(near ? s1 : 0, CROSS_7)
 *   s3 = close(s2, FULL_5);   s4 = s3 > 0.1 ? median5(s3) : s3
 *   r0[x] = the first row y with s4[y,x] > 0.1, and 0 for a column without one;  top[y,x] = y >= r0[x]
 *   s5 = (!(s4 > 0.1) && top) ? dilate(s4, FULL_9) : s4;   r0, top recomputed from s5
 *   s7 = s5; six times: s7 = (s7 < 0.1 && top) ? dilate(s7, FULL_5) : s7
 *   valid = s7 > 0.1 && top;  m = valid ? median5(s7) : s7;   f = valid ? bilateral(m, 0.5, 2.0) : m;   out = inv(f)
 * mode GDM_FILL_FAST (DIAMOND_5, extrapolate=False, blur_type='bilateral'):
 *   s1 = inv(in); s2 = dilate(s1, DIAMOND_5); s3 = close(s2, FULL_5); s5 = s3 < 0.1 ? dilate(s3, FULL_7) : s3;
 *   m = median5(s5); f = bilateral(m, 1.5, 2.0); out = inv(f)
 * stages (or NULL): f32[GDM_FILL_STAGES,B,H,W] = s1 | s2 | s3 | s4 | s5 | m | f; plane 3 is not written in the fast mode.
 * workspace: gdm_fill_depth_workspace_bytes(B, H, W, mode) bytes (0 for the fast mode, where it may be NULL).  One memset node and
 * three kernels (multiscale) or one kernel (fast), whatever B; no allocation, no host synchronisation. */
#define GDM_FILL_MULTISCALE 0
#define GDM_FILL_FAST 1
#define GDM_FILL_STAGES 7
size_t gdm_fill_depth_workspace_bytes(int B, int H, int W, int mode);
int gdm_fill_depth_hip(const float* depth, int B, int H, int W, int mode, float max_depth, void* workspace, size_t workspace_bytes,
                       float* out, float* stages, void* stream);

/* Front end, the N points of a crop and the assembled item (the loader's choose / cld_rgb_nrm / labels, datasets/lm/linemod_pbr.py:
 * 476-513, datasets/ycbv/ycbv_pbr.py:492-509) in one launch.  valid_depth f32[B,P], dpt_xyz f32[B,P,3], rgb f32[B,3,P], normals
 * f32[B,3,P], mask u8[B,P] or NULL, P = S S -> choose i32[B,N], cld_rgb_nrm f32[B,9,N], labels u8[B,N] (NULL exactly when mask is),
 * n_valid i32[B].  Which pixels are drawn is DEFINED here (no generator state, no library sort; eager, graph and forked-graph runs
 * and every build give the same points).  For crop b, pixel p in [0, P) and the 32-bit seed:
 *   valid(p)  = valid_depth[b,p] > 1e-6f                        (NaN and negative depth are invalid)
 *   key(p)    = mix(mix(mix(seed ^ 0x9e3779b9) ^ b) ^ p)        (mix = lowbias32, as for GDM_RANSAC sampling above; mix is a bijection
 *                                                                of 32-bit words, so the keys of one crop are pairwise distinct: no ties)
 *   n_valid[b] = #{p : valid(p)};   order = the valid pixels by ascending key
 *   choose[b,j] = order[j mod n_valid[b]], j < N                (a uniform subset in uniform random order when n_valid > N, the
 *                                                                wrap-around padding of np.pad(..., 'wrap') otherwise)
 *   n_valid[b] == 0:  choose[b,:] = 0                           (the reference's choose = [0], linemod_pbr.py:481-483)
 *   cld_rgb_nrm[b,0:3,j] = dpt_xyz[b,c,:], [b,3:6,j] = rgb[b,:,c], [b,6:9,j] = normals[b,:,c] with c = choose[b,j]
 *   labels[b,j] = mask[b,c] == 255 ? 1 : mask[b,c]
 * valid_depth is separate from dpt_xyz because the YCB-V item samples among the FILLED pixels and gathers the UNFILLED xyz.
 * seed_dev (or NULL): a device pointer to one word that replaces `seed` when the kernel runs, so that a captured graph can draw
 * differently on every replay.  (Restated in Python as frontend.sample_assemble_numpy.)
 * 1 <= B <= 65535, 1 <= S <= GDM_SAMPLE_MAX_S, 1 <= N <= GDM_SAMPLE_MAX_N.  workspace: device memory, 8-byte aligned, of at least
 * gdm_sample_assemble_workspace_bytes(B, S) bytes (one bit per pixel; 0 for a bad shape).  One kernel, one workgroup per crop: exact
 * selection by radix select on integer LDS histograms, no sort of all P keys, no global atomics, no allocation, no host read. */
#define GDM_SAMPLE_MAX_N 4096
#define GDM_SAMPLE_MAX_S 4096
size_t gdm_sample_assemble_workspace_bytes(int B, int S);
int gdm_sample_assemble_hip(const float* valid_depth, const float* dpt_xyz, const float* rgb, const float* normals,
                            const uint8_t* mask, int B, int S, int N, uint32_t seed, const uint32_t* seed_dev, int32_t* choose,
                            float* cld_rgb_nrm, uint8_t* labels, int32_t* n_valid, void* workspace, size_t workspace_bytes,
                            void* stream);

/* Front end, the YCB-V training item's augmentation of the CROP (datasets/ycbv/ycbv_pbr.py:468-477: rgb_add_noise, add_real_back,
 * with probability 0.2 rgb_add_noise again, normalize_color), between gdm_warp_crop_hip and gdm_fill_depth_hip.  rgb f32[B,3,S,S]
 * as gdm_warp_crop_hip wrote it, depth f32[B,S,S], mask u8[B,S,S] -> out_rgb f32[B,3,S,S], out_depth f32[B,S,S] (neither may alias
 * an input).  Everything between the first and the last line below is integer arithmetic on uint8 levels and is DEFINED here
 * operation by operation (frontend.augment_crops_numpy restates it; the kernel equals it bit for bit; parity with a cv2 build or
 * with np.random streams is not claimed).  `/` is the quotient of non-negative integers, `>>` the arithmetic shift
 * (a floor), clip(v) = min(255, max(0, v)).
 *   levels    v_c = (int) rintf(min(255, max(0, ((x_c std_c) + mean_c) 255.0f)))    (NaN -> 0; exact for a crop: 1.5e-5 from an integer)
 *   normalise x_c = (((float) v_c / 255.0f) - mean_c) / std_c                      (the three fp32 operations of gdm_warp_crop_hip,
 *                                                                                   mean .485 .456 .406, std .229 .224 .224)
 * DRAWS.  mix = lowbias32 as above;  hb = mix(mix(seed ^ 0x85ebca6b) ^ b);  decision word D(k) = mix(hb ^ k), k < 256;
 *   below(w, n) = ((uint64) w n) >> 32;  "with probability 0.2" = w > 0xcccccccc;  "with probability 0.8" = w > 0x33333333
 *   pixel word of pass q, noise stream e, pixel p = y S + x, channel c:  mix(mix(hb ^ (256 + 2 q + e)) ^ (3 p + c))
 *   pass q in {0, 1} uses k = 16 q + j:
 *     j 0  ks = 320 + below(D, 52)          saturation gain in 1/256 (1.25 .. 1.45)
 *       1  kv = 294 + below(D, 52)          value gain in 1/256 (1.15 .. 1.35)
 *       2  sharpen with probability 0.2;    3  u = D >> 24: the centre weight is c = 9 + 3 u / 256
 *       4  motion blur with probability 0.2;  5  angle = below(D, 360) degrees;  6  length L = below(D, 15) + 1
 *       7  Gaussian blur with probability 0.2;  8  3 x 3 with probability 0.8, else 5 x 5;  9  sigma level l = D >> 24
 *       10 noise range n = 15 with probability 0.8, else 25;  11 sigma = below(D, n);  12 further noise of sigma 7 with probability 0.2
 *   k = 32: a second pass with probability 0.2;  33: bank frame n = D mod Nb;  34: wy = D mod (Hb - S - 1);  35: wx = D mod (Wb - S - 1)
 * ONE PASS, in this order, every stage on all three channels of the whole S x S image (a tap outside it reads the pixel reflected
 * about the border pixel, BORDER_REFLECT_101: -i -> i, S - 1 + i -> S - 1 - i):
 *   1 gain     M = max_c v_c, m = min_c v_c, d = M - m;  M' = min(255, (M kv) >> 8);  s = M > 0 ? (255 d + (M >> 1)) / M : 0;
 *              s' = min(255, (s ks) >> 8);  m' = M' - (M' s' + 127) / 255;
 *              v_c' = d > 0 ? m' + ((v_c - m) (M' - m') + (d >> 1)) / d : M'     (the hue, i.e. the ratio of the middle channel, is kept:
 *              cv2 would quantise it to 0 .. 180; S and V are symmetric in the channels, so the loader's BGR/RGB mix-up is immaterial)
 *   2 sharpen  c256 = 2304 + 3 u, q = 256 + 3 u (= c256 - 2048);  t = 2 (c256 v - 256 (sum of the 8 neighbours)) + q;
 *              v' = t < 0 ? 0 : min(255, t / (2 q))                               (round to nearest, saturate)
 *   3 motion   cs = gdm_aug_cos_q14[angle], sn = gdm_aug_cos_q14[(angle + 270) mod 360] (csrc/gdm_augment_tables.h, rint(16384 cos));
 *              a = (max(|cs|, |sn|) L 2) >> 14 (1 <= a <= 30; a <= 0 would leave the image as it is);  cx = a / 2;
 *              ex = cx + trunc(cs L / 16384), ey = cx + trunc(sn L / 16384) (trunc towards zero);  the taps are the points of the
 *              integer Bresenham line from (cx, cx) to (ex, ey) that lie inside [0, a)^2 (what cv2.line draws into the a x a kernel):
 *                dx = |ex - cx|, sx = sign, dy = -|ey - cx|, sy = sign, err = dx + dy;  repeat { plot (x, y); stop at (ex, ey);
 *                e2 = 2 err;  if (e2 >= dy) { err += dy; x += sx; }  if (e2 <= dx) { err += dx; y += sy; } }
 *              a tap (x, y) reads pixel (row + y - cx, column + x - cx);  n taps (1 <= n <= 16):  v' = (sum + (n >> 1)) / n
 *   4 Gaussian w = gdm_aug_gauss3[l] or gdm_aug_gauss5[l] (weights w_|i| summing to 256 over a row);
 *              v' = (sum_{i,j} w_|i| w_|j| v[y+i, x+j] + 32768) >> 16
 *   5 noise    z(word) = (sum of its four bytes) - 510 (Irwin-Hall, standard deviation 147.8, tails end at 3.45 sigma);
 *              v' = clip(v + ((z(word of stream 0) sigma 443 + 32768) >> 16));  with further noise then
 *              v'' = clip(v' + ((z(word of stream 1) 7 443 + 32768) >> 16))
 * PASTE (add_real_back; only with a bank: bg_rgb u8[Nb,Hb,Wb,3], bg_depth f32[Nb,Hb,Wb] in metres, bg_mask u8[Nb,Hb,Wb], all three
 * or none, Hb, Wb >= S + 2): keep = bg_mask[n, wy+y, wx+x] < 255;
 *   rgb   = mask[b,y,x] > 0 ? rgb : (keep ? bg_rgb[n, wy+y, wx+x, :] : 0)
 *   depth = depth[b,y,x] > 1e-6f ? depth : (keep ? bg_depth[n, wy+y, wx+x] : 0.0f)        (without a bank out_depth = depth)
 * THE CALL: levels, pass 0, paste, with probability 0.2 pass 1, normalise.  enable u8[B] or NULL: a crop with enable[b] == 0 is
 * copied bit for bit (the loader's img_typ == 'synt' condition).  seed_dev as for gdm_sample_assemble_hip.  dpt_xyz is no argument:
 * the loader gathers cld from the unaugmented crop.
 * 1 <= B <= 65535, GDM_AUG_MIN_S <= S <= GDM_AUG_MAX_S (a blur reaches 15 pixels: one reflection needs S >= 32).  workspace: the uint8
 * image between the passes, gdm_augment_workspace_bytes(B, S) bytes (0 for a bad shape), 4-byte aligned.  Two launches whatever B: one
 * workgroup per (crop, 32 x 32 tile) keeps the tile and the halo its crop's drawn stages need (0 .. 18 pixels) in LDS and recomputes
 * the halo; no allocation, no host read, no atomics. */
#define GDM_AUG_MIN_S 32
#define GDM_AUG_MAX_S 4096
size_t gdm_augment_workspace_bytes(int B, int S);
int gdm_augment_crops_hip(const float* rgb, const float* depth, const uint8_t* mask, const uint8_t* bg_rgb, const float* bg_depth,
                          const uint8_t* bg_mask, const uint8_t* enable, int B, int S, int Nb, int Hb, int Wb, uint32_t seed,
                          const uint32_t* seed_dev, float* out_rgb, float* out_depth, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Measurement aid (tools/augment_profile.py): while on != 0, later gdm_augment_crops_hip calls of this process apply sharpen, motion
 * blur, Gaussian blur and the second pass to EVERY crop, their parameters drawn as usual -- the cost of the heaviest item, not a result
 * the rule above defines.  Off by default. */
void gdm_augment_force_all_stages(int on);
/* The loader's aug_bbox_DZI (datasets/lm/linemod_pbr.py:99-120) with counter-based draws: bbox f32[B,4] = (x1,y1,x2,y2) ->
 * center f32[B,2], scale f32[B].  fp32, one rounding per operation, in this order:
 *   bw = x2 - x1, bh = y2 - y1, cx = 0.5 (x1 + x2), cy = 0.5 (y1 + y2), m = bh > bw or bh is NaN ? bh : bw
 *   train == 0:  scale = m pad_ratio
 *   train != 0:  u_k = 2 ((float) (w_k >> 8) 2^-24) - 1 (exact), w_k = mix(mix(mix(seed ^ 0xc2b2ae35) ^ b) ^ k), k = 0, 1, 2;
 *                cx = cx + bw (shift_ratio u_1), cy = cy + bh (shift_ratio u_2), scale = (m (1 + scale_ratio u_0)) pad_ratio
 *   scale = scale > max_side ? max_side : scale
 * (frontend.dzi_boxes_numpy restates it; frontend.dzi_boxes(jitter="torch") is the same arithmetic on torch.rand draws.) */
int gdm_dzi_boxes_hip(const float* bbox, int B, float max_side, float pad_ratio, float scale_ratio, float shift_ratio, int train,
                      uint32_t seed, const uint32_t* seed_dev, float* center, float* scale, void* stream);

/* ---- training-mode BatchNorm (+ ReLU / LeakyReLU), forward and backward -------------------------------------------------------
 * Replaces the conv -> nn.BatchNorm{1,2}d -> activation chains of the embedding network in the training step
 * (models/pytorch_utils.py:70-124, models/RandLA/pytorch_utils.py:34-105, models/cnn/extractors.py:36-58; train_lm.py:171-225).
 * x, y, grad f32[B,C,inner] contiguous (inner % 4 == 0, B*C <= 65535, 16-byte aligned).  sums: double[gdm_bn_sums_len(B,C,inner)] =
 * G partial pairs per channel of (sum x, sum x^2) -- or (sum g', sum g' x) in the backward, g' = grad * act'(.) -- then the element
 * count per channel and G; no atomics, no memset, the apply calls add the partials (`groups` = 0: the layout the reduce call of the
 * same shape wrote).  A data-parallel caller (SyncBatchNorm semantics, /root/reference/train_lm.py:412) folds the partials to one
 * pair per channel, all-reduces pairs and count, and passes that buffer -- double[2C+1]: pairs, count -- with `groups` = 1.
 * saved f32[5C] = a | b | m | rstd | mean - m with y = act(a (x - m) + b), m the batch mean rounded to fp32; written by the forward
 * apply, read by both backward calls.
 * act: 0 none, 1 ReLU, 2 LeakyReLU(slope).  running_mean / running_var (both or neither) are updated with `momentum`. */
long gdm_bn_sums_len(int B, int C, long inner);
int gdm_bn_stats_hip(const float* x, int B, int C, long inner, double* sums, void* stream);
int gdm_bn_fwd_apply_hip(const float* x, const double* sums, int groups, const float* weight, const float* bias, int B, int C, long inner, float eps,
                         float momentum, int act, float slope, float* saved, float* running_mean, float* running_var, float* y, void* stream);
int gdm_bn_bwd_reduce_hip(const float* x, const float* grad_out, const float* saved, int B, int C, long inner, int act, float slope,
                          double* sums, void* stream);
int gdm_bn_bwd_apply_hip(const float* x, const float* grad_out, const double* sums, int groups, const float* weight, const float* saved, int B, int C,
                         long inner, int act, float slope, float* grad_weight, float* grad_bias, float* grad_x, void* stream);

/* ---------------------------------------------------------------------------------------
 * The per-point heads of GeoMatch.forward in one kernel (inference; /root/reference/models/geoMatch.py:159-200: feature_encoding_layer,
 * normalize_feature_layer, the residual add and seg_layer -- nine 1x1 convolutions per scene point).  Input x0 = channels of a
 * f32[B,Ca,N] followed by b f32[B,128-Ca,N] (b may be NULL when Ca == 128).  `nlayer` hidden layers 128 -> 128:
 *   x_{l+1} = act_l(scale_l * (W_l x_l) + shift_l)  [+ r after layer res_layer];  out_feat f32[B,128,N] = the affine output of layer
 *   feat_layer (before the residual);  then out_last f32[B,c_last,N] = W_last x_nlayer + shift_last (c_last <= 16).
 * The residual r is given as the input is, by (ra, rb, rCa); NULL ra = the input x0.
 * w[l], w_last: weights packed by gdm_conv1x1_pack_weight_hip(Cout, 128) (rows padded to 128); scale[l] / shift[l] may be NULL (1 / 0);
 * act[l]: 0 none, 1 ReLU; feat_layer / res_layer: -1 = none.  w, scale, shift, act are HOST arrays of nlayer entries.
 * c_last = 0 ends the chain with its hidden layers (w_last / out_last unused); out_feat may be NULL with feat_layer < 0.
 * GeoMatch.forward runs the chain in two pieces, the four feature layers first and the normalise / segmentation layers second, so that
 * the matching kernel -- which reads the features only -- runs beside the second piece.
 * Split-bf16 products (hi*hi + hi*lo + lo*hi), fp32 accumulate, as the convolution kernels. */
int gdm_point_heads2_hip(const float* a, const float* b, int Ca, const float* ra, const float* rb, int rCa, int B, int N, int nlayer,
                         const void* const* w, const float* const* scale, const float* const* shift, const int* act, int feat_layer,
                         int res_layer, const void* w_last, const float* shift_last, int c_last, float* out_feat, float* out_last,
                         void* stream);
/* The same with one more output: out_rows u8[B*N, 512] (may be NULL), the matching kernel's split-bf16 operand rows of out_feat -- byte
 * for byte what gdm_match_pack_hip(out_feat, B, 128, N, GDM_MATCH_BF16X3, out_rows) writes, formed from the kernel's own accumulators
 * (the norm and the row write are the pack kernel's code, csrc/gdm_match_rows.h), so that no pack launch stands between the heads and
 * gdm_match_packed_hip.  It needs feat_layer >= 0 and a 16-byte aligned buffer of gdm_match_rows_bytes(B * N) bytes.  out_feat and
 * out_last do not depend on whether the rows are asked for. */
int gdm_point_heads3_hip(const float* a, const float* b, int Ca, const float* ra, const float* rb, int rCa, int B, int N, int nlayer,
                         const void* const* w, const float* const* scale, const float* const* shift, const int* act, int feat_layer,
                         int res_layer, const void* w_last, const float* shift_last, int c_last, float* out_feat, float* out_last,
                         void* out_rows, void* stream);

/* ---------------------------------------------------------------------------------------
 * One per-point (1x1) layer in a single launch (inference): concat-free, BatchNorm / bias / activation / residual branch folded in.
 * Replaces torch.cat -> Conv1d/Conv2d(1x1) -> BatchNorm -> activation of /root/reference/models/pytorch_utils.py:70-124 and
 * models/RandLA/pytorch_utils.py:34-99, the tail lrelu(mlp2(f) + shortcut(x)) of Dilated_res_block (RandLANet.py:685-688), the
 * fusion layers over cat(point, pooled pixel) features (ffb6d.py:224-231,259-265) and the decoder layers over
 * cat(skip, nearest_interpolation(deeper)) (ffb6d.py:246-250,268-272; the interpolation = `idx` of the second segment).
 *   out[b, out_c0 + c, i] = act( scale[c] * sum_k wt[k][c] * X[b,k,i] + shift[c] )
 * X = the channels of segs[0], segs[1], ... in order (the concat, never formed; nseg in [1,4], four only when K >= 32).  A segment is f32[B,C,n_src]
 * channel-major, read at column i (n_src == n) or at idx[b*n + i] (i32, any n_src).  A residual branch
 * s1*(W1 . x1) + b1 + s2*(W2 . x2) + b2 is the two-segment layer with wt = [s1*W1^T ; s2*W2^T], shift = b1 + b2 (the caller folds).
 * wt f32[K,Cout] TRANSPOSED weight (w_rowmajor = 0), K = sum of the segments' C; or, with w_rowmajor != 0, wt f32[Cout,K] as the
 * module holds it (nn.Conv1d / nn.Conv2d 1x1 weight), so that the TRAINING forward W . x and input gradient W^T . go (wt = the same
 * tensor read as [K' = Cout][Cout' = K], w_rowmajor = 0) of /root/reference/models/pytorch_utils.py:70-124 need no transposed copy of
 * a weight that changes every step.  scale / shift f32[Cout] or NULL (1 / 0).
 * act: 0 none, 1 ReLU, 2 leaky ReLU (slope).  out f32[B,out_C,n] (point_major 0) or f32[B*n,out_C] (1), 16-byte aligned;
 * channels [out_c0, out_c0 + Cout) of it are written.  fp32 FMAs; the K axis may be summed as up to four partial sums added in
 * fixed order (deterministic; no atomics). */
typedef struct {
    const float* x;
    const int32_t* idx;
    int32_t C, n_src;
} gdm_pw_seg;
int gdm_pointwise2_hip(const gdm_pw_seg* segs, int nseg, const float* wt, int w_rowmajor, const float* scale, const float* shift,
                       int B, int n, int Cout, int act, float slope, float* out, int out_C, int out_c0, int point_major, void* stream);
/* Up to four independent plain layers out_j f32[B,Cout,n_j] = W_j^T . x_j (x_j f32[B,K,n_j], wt_j f32[K,Cout]; no scale / shift /
 * activation) of equal K >= 32 and Cout in ONE launch: the four prior products of the pyramid-pooling module
 * (/root/reference/models/cnn/pspnet.py:17-31, `stage(feats)` of the 1 / 2 / 3 / 6-bin pools folded with the bottleneck's slices).
 * Bit-identical to njobs calls of gdm_pointwise2_hip (w_rowmajor = 0): jobs that would take different K splits alone (gdm_pointwise2_hip
 * picks the split from a job's own grid size) are launched apart, one launch per distinct split. */
typedef struct {
    const float* x;
    const float* wt;
    float* out;
    int32_t n;
} gdm_pw_job;
int gdm_pointwise_jobs_hip(const gdm_pw_job* jobs, int njobs, int B, int K, int Cout, void* stream);
/* Two chained narrow per-point layers in one launch, both results written: y0 = act0(s0 (W0 x) + b0) f32[B,C1,n],
 * y1 = act1(s1 (W1 y0) + b1) f32[B,C2,n]; x f32[B,C0,n], w0t f32[C0,C1], w1t f32[C1,C2] (weights transposed), s / b folded
 * BatchNorm or NULL, act 0 none / 1 ReLU / 2 LeakyReLU(slope); C0, C1 <= 16, C2 <= 32.  The RandLA stem fc0 and the first block's
 * mlp1 (/root/reference/models/RandLA/RandLANet.py:19,683-684).  Bit-identical to two gdm_pointwise2_hip launches. */
int gdm_pointwise_chain2_hip(const float* x, const float* w0t, const float* s0, const float* b0, int act0, float slope0,
                             const float* w1t, const float* s1, const float* b1, int act1, float slope1,
                             int B, int n, int C0, int C1, int C2, float* y0, float* y1, void* stream);

/* ---------------------------------------------------------------------------------------
 * The ResNet stem in one launch (inference): conv 7x7 / stride 2 / pad 3 (3 -> 64, no bias) + scale / shift (folded BatchNorm) +
 * ReLU + max-pool 3x3 / stride 2 / pad 1 (/root/reference/models/cnn/extractors.py:112-116,181-185: conv1, bn1, relu, maxpool).
 * x f32[B,3,H,W] -> out f32[B,64,PH,PW] (PH = ((H-1)/2)/2 + 1, PW likewise) and / or out_packed = the split-bf16 operand planes of
 * the next 3x3 convolution (gdm_conv3x3_act_bytes(B, 64, PH, PW) bytes, zero border already in place); either may be NULL.
 * wpk: gdm_stem_pack_weight_hip of w f32[64,3,7,7] (gdm_stem_weight_bytes() bytes).  Split-bf16 products, fp32 accumulate. */
size_t gdm_stem_weight_bytes(void);
int gdm_stem_pack_weight_hip(const float* w, void* wpk, void* stream);
int gdm_stem_hip(const float* x, const void* wpk, const float* scale, const float* shift, int B, int H, int W, float* out,
                 void* out_packed, void* stream);

/* ---------------------------------------------------------------------------------------
 * Weight gradient of a 3x3 / stride 1 / pad 1 convolution on the split-bf16 MFMA GEMM (training; backward of
 * /root/reference/models/cnn/extractors.py:36-58): dW[co,ci,ky,kx] = sum_{b,y,x} go[b,co,y,x] * x[b,ci,y+ky-1,x+kx-1] is the GEMM
 * GO (Cout x pixels) . X_tap^T (pixels x Cin).  These two kernels re-lay the operands for gdm_conv1x1_packed_hip: the contraction (its
 * "Cin") runs over the B*H*W pixels in chunks of 128, its "pixels" are the 9 x Cin grid of (tap, ci), its "weights" the rows of go.
 *   xpk = gdm_wgrad_pack_x_hip(x f32[B,Cin,H,W])   gdm_wgrad_x_bytes(B,Cin,H,W) bytes (the tap shift applied here, zero outside the map)
 *   gpk = gdm_wgrad_pack_go_hip(go f32[B,Cout,H,W]) gdm_wgrad_go_bytes(B,Cout,H,W) bytes
 * then ONE launch of the GEMM with per-image weights, its "images" being P equal parts of n = B*H*W/128/P chunks of the contraction,
 *   gdm_conv1x1_packed_wb_hip(xpk, gpk, n*CoutP*512, P, 128*n, Cout, 9, Cin, parts, stream)      (9*Cin % 256 == 0)
 * gives parts f32[P, Cout, 9, Cin]; dW = their sum over P, permuted to [Cout, Cin, 3, 3].  (Or any chunk range [c0, c0+n) alone:
 * gdm_conv1x1_packed_hip(xpk + c0*32*11*(Cin+2)*16, gpk + c0*CoutP*512, NULL, NULL, 1, 128*n, Cout, 9, Cin, 0, 0, part, stream).)
 * W in {32, 64}, H*W % 128 == 0, Cin % 32 == 0; CoutP = Cout rounded up to 128.  Both byte counts are 0 for an unsupported shape. */
size_t gdm_wgrad_x_bytes(int B, int Cin, int H, int W);
size_t gdm_wgrad_go_bytes(int B, int Cout, int H, int W);
int gdm_wgrad_pack_x_hip(const float* x, int B, int Cin, int H, int W, void* out, void* stream);
int gdm_wgrad_pack_go_hip(const float* go, int B, int Cout, int H, int W, void* out, void* stream);
/* The 1x1 case, dW[co,ci] = sum_{b,p} go[b,co,p] * x[b,ci,p] (x f32[B,Cin,P], P % 128 == 0, Cin % 32 == 0): xpk = gdm_wgrad_pack_x1_hip
 * (gdm_wgrad_x1_bytes bytes), gpk = gdm_wgrad_pack_go_hip(go, B, Cout, P/32, 32), then
 * gdm_conv1x1_packed_wb_hip(xpk, gpk, n*CoutP*512, parts, 128*n, Cout, 1, Cin, out f32[parts, Cout, Cin], stream) (Cin % 256 == 0). */
size_t gdm_wgrad_x1_bytes(int B, int Cin, int P);
int gdm_wgrad_pack_x1_hip(const float* x, int B, int Cin, int P, void* out, void* stream);
/* Measurement aid: `blocks` workgroups of 8 waves, each wave `iters` x 8 independent v_mfma_f32_16x16x32_bf16 on registers (no memory):
 * the rate the matrix pipe sustains on this chip at the clock it holds under that load.  flops = blocks*8*iters*8*16384.  chain = 1: no
 * MFMA depends on its predecessor; chain = 3: three consecutive MFMAs into one accumulator (a split-bf16 product issued back to back). */
int gdm_mfma_probe_hip(int blocks, int iters, int chain, float* sink, void* stream);
/* The same loop with the B operands re-read from LDS: rpu (1, 2, 4) ds_read_b128 per 12 MFMAs (4 = the convolution kernel's ratio).
 * flops = blocks*8*iters*12*16384. */
int gdm_mfma_probe_lds_hip(int blocks, int iters, int rpu, float* sink, void* stream);
/* Small-channel form with no re-layout pass (HBM-bound; the 1x1 layers of the 32 / 64-channel full-resolution stages and of the point
 * branch under training): partial[s][co][ci] = sum over the s-th of nsplit slices of the B*P/32 pixel steps of go[b,co,p] * x[b,ci,p]
 * (rows of P floats, batch strides in elements, P % 32 == 0, split-bf16 MFMA); bias_partial[s][co] (optional) = the row sums of go.
 * The caller adds the nsplit partials. */
int gdm_wgrad_direct_hip(const float* go, long go_bstride, const float* x, long x_bstride, int B, int Cout, int Cin, int P,
                         int nsplit, float* partial, float* bias_partial, void* stream);
/* gdm_conv1x1_packed_hip without epilogue, NCHW output, with the weights of image b at wpk + b*w_bstride (H*W % 256 == 0).  The operand
 * limit (at gdm_conv3x3_packed_hip) counts all B weight sets: for the weight-gradient GEMMs above, gdm_wgrad_x_bytes / gdm_wgrad_x1_bytes
 * and gdm_wgrad_go_bytes must each stay below 2 GiB, or the call is refused on the host. */
int gdm_conv1x1_packed_wb_hip(const void* xpk, const void* wpk, long w_bstride, int B, int Cin, int Cout, int H, int W, float* out,
                              void* stream);

/* ---------------------------------------------------------------------------------------
 * Batched strided copies of 4-byte words (f32 / i32), one launch for a table of views: job i fills the dense array
 * dst[B][R1][R2][E] from src[b*sb + r1*s1 + r2*s2 + e] (strides in words).  The neighbour pyramid uses it for the strided xyz
 * grids (datasets/lm/linemod_pbr.py:517-527: R1 x R2 = rows x columns at stride sr), the prefix sub-clouds (:538) and the pooling
 * index prefixes, which the reference makes with numpy slicing + copies in the DataLoader worker. */
typedef struct gdm_copy_job {
    void* dst;
    const void* src;
    int64_t sb, s1, s2;
    int32_t B, R1, R2, E;
} gdm_copy_job;
#define GDM_COPY_MAX_JOBS 16
int gdm_copy_jobs_hip(const gdm_copy_job* jobs /* host array */, int njobs, void* stream);

/* ---------------------------------------------------------------------------------------
 * BOP pose errors (/root/reference/lib/pysixd/pose_error.py:22-179 with misc.py:206-254,511-525,571-590 and visibility.py:9-74).
 * All arithmetic that decides a result is fp64; lengths are in the caller's unit.  K is f64[3,3] (k_per_instance 0) or f64[n,3,3] (1).
 *
 * MSSD and MSPD (pose_error.py:131-179) of n pose pairs of one object: for symmetry s the ground truth is (R_gt S_R[s],
 * R_gt S_t[s] + t_gt); mssd[i] = min_s max_p |P_est p - P_gt,s p|, mspd[i] = min_s max_p |proj(P_est p) - proj(P_gt,s p)| with
 * proj(X) = (K X)[:2] / (K X)[2] (misc.project_pts); best_sym_* i32[n] = the minimising s, the first one on a tie.
 * RT_est, RT_gt f64[n,3,4]; pts f64[M,3]; sym_R f64[S,3,3]; sym_t f64[S,3]; err f64[2,n,S] = the per-symmetry maxima (MSSD rows
 * first), the only temporary: no [n,S,M] array is formed. */
int gdm_mssd_mspd_hip(const double* RT_est, const double* RT_gt, const double* pts, const double* sym_R, const double* sym_t,
                      const double* K, int k_per_instance, int n, int M, int S, double* err, double* mssd, double* mspd,
                      int32_t* best_sym_mssd, int32_t* best_sym_mspd, void* stream);
/* Depth images of one triangle mesh in n poses (what pose_error.py:59-64 asks of its `renderer`): depth f32[n,H,W], 0 where nothing
 * is drawn.  verts f32[V,3] (verts_f64 0) or f64[V,3] (1); faces i32[F,3]; RT f64[n,3,4].  THE PIXEL RULE (pixel_rule.py restates
 * it for evaluation.render_depth_numpy; csrc/gdm_raster.h holds its device code):
 *   vertex      P = R v + t in fp64, each component ((R_i0 x + R_i1 y) + R_i2 z) + t_i
 *   projection  u = fx (X / Z) + cx, v = fy (Y / Z) + cy with fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2]; skew is ignored.
 *               Pixel centres sit at integer coordinates.
 *   discard     the whole triangle when a vertex index lies outside [0, V), a vertex has Z <= near, or |u| or |v| above 2^16, or its
 *               snapped area is 0
 *   snapping    Xs = (int64) floor(u * 256 + 0.5), Ys likewise
 *   coverage    int64 edge functions at (256 px, 256 py), the winding normalised by the sign of the area (no culling); a pixel is
 *               covered when all three are >= 0, a zero counting only on a top or left edge (dy < 0, or dy == 0 and dx > 0, of the
 *               normalised winding); the pixel range is the snapped bounding box clamped to the image
 *   depth       iz = ((w0 (1/z0) + w1 (1/z1)) + w2 (1/z2)) / A, w_i the edge value opposite vertex i, A their sum; d = (float)(1 / iz)
 *   z-buffer    the minimum over the triangles (unsigned atomicMin on the fp32 bit pattern: reproducible), cleared to +inf;
 *               untouched pixels become 0 at the end -- or stay +inf with keep_inf != 0, for gdm_vsd_counts_hip(inf_is_empty = 1). */
int gdm_render_depth_hip(const void* verts, int verts_f64, const int32_t* faces, const double* RT, const double* K, int k_per_instance,
                         int n, int V, int F, int H, int W, double near, int keep_inf, float* depth, void* stream);
/* The integer counts the VSD errors are made of (pose_error.py:84-126, visib_mode "bop19"): counts i32[n, 2 + T] = (union, inter,
 * cost_0 .. cost_{T-1}) with cost_j = #{inter pixels with |dist_gt - dist_est| (/ diameter when diameter > 0) >= taus[j]}; the error is
 * (cost_j + union - inter) / union, 1 for an empty union.  depth_est, depth_gt f32[n,H,W]; depth_test f32[H,W] (test_per_instance 0)
 * or f32[n,H,W] (1); distance images fp64 sqrt((px d)^2 + (py d)^2 + d^2), px = (col - cx) / fx; the visibility test is the fp32
 * difference of the fp32-cast distances <= (float) delta, or a missing test depth.  taus: HOST array f64[T], T <= GDM_VSD_MAX_TAUS.
 * tl_sums f64[n,T] or NULL: the sums of min(dist / tau, 1) of cost_type "tlinear" (fp64 atomic adds of per-workgroup sums: the last
 * bits depend on their order; the counts are exact).  inf_is_empty != 0: +inf in depth_est / depth_gt reads as 0. */
#define GDM_VSD_MAX_TAUS 16
int gdm_vsd_counts_hip(const float* depth_est, const float* depth_gt, const float* depth_test, int test_per_instance, const double* K,
                       int k_per_instance, int n, int H, int W, double delta, const double* taus /* host array */, int T,
                       double diameter, int inf_is_empty, int32_t* counts, double* tl_sums, void* stream);
/* Pose candidates verified against the observed depth (pose.verify_poses_numpy restates it bit for bit): C candidate
 * poses of one mesh for each of n instances are rasterised by THE PIXEL RULE above into tiles of the instance's window held in LDS,
 * compared there with the observed depth, and summed into six integers per candidate; no depth image is written.  Parity with any
 * other verifier is NOT claimed.  verts, faces as for gdm_render_depth_hip; RT f64[n,C,3,4]; depth_obs f32[n,H,W]
 * (obs_per_instance 1) or one shared f32[H,W] (0); window i32[n,4] = (x0, y0, x1, y1), inclusive, in frame pixels -- DEVICE data the
 * entry does not read: the kernel clamps it to the frame, an empty one gives all-zero counts -- or NULL for the whole frame;
 * cand_valid u8[n,C] or NULL (every candidate valid).  THE VERIFICATION RULE for a pixel p of the clamped window whose rendered depth
 * z_r is drawn (the z-buffer minimum of the candidate, below +inf), with z_o = depth_obs[p]; all fp32, single operations:
 *   NODEPTH     z_o is not > 0 (zero, negative, NaN)
 *   otherwise   d = z_o - z_r, a = |d|, D = (float) delta
 *   AGREE       a <= D; q += (int) floor(a * Q) with Q = (float)(256.0 / delta) formed on the host: 0 for a perfect pixel, 256 at the edge
 *   FRONT       d < -D: something stands in front of the model (occlusion, neutral)
 *   BEHIND      d > D: the camera sees through the model (a contradiction)
 * counts i32[n,C,6] = (n_model, n_agree, n_front, n_behind, n_nodepth, q_agree), n_model the sum of the four classes; integer atomic
 * adds, cleared by the entry: reproducible bit for bit.
 * THE SELECTION, fp64, candidates in index order:
 *   score[i,c] = (n_agree - q_agree / 512.0) / max(1.0, (n_agree + n_behind) + front_weight * n_front), written for every candidate;
 *   candidate c is eligible when cand_valid[i,c] != 0 and n_model >= min_px; best[i] = the eligible candidate with the largest score,
 *   the lowest index on a tie, -1 when none is eligible.
 * LIMITS (refused beyond): n, C <= 65535, H, W <= 16384, H W <= 2^22 (q_agree stays inside an int32), tiles n C <= 2^23 with
 * tiles = ceil(W / 64) ceil(H / 64); near >= 0, delta > 0 with delta and 256 / delta finite in fp32, front_weight >= 0, min_px >= 0.
 * No workspace, no allocation and no host read: the call captures in a hipGraph. */
int gdm_pose_verify_hip(const void* verts, int verts_f64, const int32_t* faces, const double* RT, const double* K, int k_per_instance,
                        const float* depth_obs, int obs_per_instance, const int32_t* window, const uint8_t* cand_valid, int n, int C,
                        int V, int F, int H, int W, double near, double delta, double front_weight, int min_px, int32_t* counts,
                        double* score, int32_t* best, void* stream);
/* Pose candidates refined against the observed depth by render-and-compare (pose.refine_poses_depth_numpy restates it
 * operation for operation).  Where verification only counts, this entry moves a pose towards the frame: `iters` Gauss-Newton
 * iterations on the point-to-plane residual between every agreeing depth pixel and the mesh face drawn at it.  Parity with any other
 * depth refiner is NOT claimed; reject, huber and min_cos are the defaults of a definition, not tuned values.  verts, faces, K,
 * depth_obs, window, cand_valid, n, C, V, F, H, W, near as for gdm_pose_verify_hip; RT_in f64[n,C,3,4] (object to camera).
 * THE DEPTH REFINEMENT RULE, one iteration of candidate c of instance i whose status is 0, with pose [R | t] (fp64):
 *   rasterise   the mesh under [R | t] by THE PIXEL RULE above (set-up with the frame's H, W) into the window clamped to the frame;
 *               per pixel the minimum of the 64-bit key (fp32 depth bits << 32) | face index: the nearest face, the lowest face index
 *               among equal depth bits (the key of gdm_render_frames_hip, here in LDS).  z_r = the key's depth.
 *   pair        a drawn pixel (col u, row v) with z_o = depth_obs[v, u] pairs when, in fp32 single operations, z_o > 0 and
 *               |z_o - z_r| <= (float) reject.  (What verification calls FRONT, BEHIND or NODEPTH pulls on nothing.)
 *   terms       fp64, the library is built with -ffp-contract=off; zo = (double) z_o:
 *               o = ((zo (u - cx)) / fx, (zo (v - cy)) / fy, zo);  d = o - t;  x_j = (R_0j d_0 + R_1j d_1) + R_2j d_2  (x = R^T (o - t))
 *               v0, v1, v2 = the face's vertices in stored order, widened from fp32 where the mesh is fp32; e1 = v1 - v0, e2 = v2 - v0;
 *               m = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x);  mm = (mx mx + my my) + mz mz; no pair unless mm > 0;
 *               n = m / sqrt(mm) (the sign of n cancels in every sum: no orientation step)
 *               grazing gate, only with min_cos > 0: q_i = (R_i0 nx + R_i1 ny) + R_i2 nz; the pair is dropped when
 *               |(q0 ox + q1 oy) + q2 oz| < min_cos sqrt((ox ox + oy oy) + oz oz)
 *               r = (nx (x0 - v0x) + ny (x1 - v0y)) + nz (x2 - v0z);  w = 1, or huber / |r| when huber > 0 and |r| > huber
 *               J = (x1 nz - x2 ny, x2 nx - x0 nz, x0 ny - x1 nx, nx, ny, nz)
 *   sums        the 29 sums of gdm_icp_plane_update_hip -- A += (w J_p) J_q for p <= q (21), g_p += (w J_p) r (6), S += w,
 *               L2 += w ((x0 x0 + x1 x1) + x2 x2) --, E += |r| and the integer pair count, per (tile of the window) in a fixed order,
 *               then over the window's tiles in tile index order.  No floating-point atomics: reproducible bit for bit.
 *   solve       pairs < max(min_px, 6): status 2.  Otherwise the solve, the degeneracy test (a scaled pivot below pivot_min: status 3)
 *               and the composition R <- R exp([omega]x)^T, t <- t - R_new v of gdm_icp_plane_update_hip, the same statements.
 *   stop        iters += 1; mean = E / pairs; |err - mean| < tolerance: status 1; err <- mean  (err starts at 0).
 * The pose stays fp64 from iteration to iteration.  status i32[n,C]: 0 still active after `iters` iterations, 1 converged by the stop
 * rule, 2 starved, 3 degenerate, 4 cand_valid == 0 on entry; 2, 3 and 4 leave the pose of that moment as it is (bit-identical to
 * RT_in when they arise in the first iteration), and a candidate whose status is not 0 is not touched again.  OUTPUTS RT f64[n,C,3,4],
 * status, iters_out i32[n,C] (iterations applied), err f64[n,C] (mean |r| of the last applied iteration, 0 before one),
 * pairs i32[n,C] (of the last iteration evaluated).
 * workspace: gdm_pose_refine_depth_workspace_bytes(n, C, H, W) = n C ceil(W / 64) ceil(H / 64) 32 doubles (one row of 30 sums, the
 * pair count and a zero per tile a window can have; 0 for arguments the entry refuses), 8-byte aligned.  1 + 2 iters launches; no
 * allocation, no host read, no memset node: the call captures in a hipGraph.
 * LIMITS (refused beyond, before any HIP call): those of gdm_pose_verify_hip; iters in [1, 64]; reject > 0 and finite in fp32;
 * huber >= 0 (0: off); 0 <= min_cos < 1 (0: off); min_px >= 0; tolerance >= 0; pivot_min > 0. */
size_t gdm_pose_refine_depth_workspace_bytes(int n, int C, int H, int W);
int gdm_pose_refine_depth_hip(const void* verts, int verts_f64, const int32_t* faces, const double* RT_in, const double* K,
                              int k_per_instance, const float* depth_obs, int obs_per_instance, const int32_t* window,
                              const uint8_t* cand_valid, int n, int C, int V, int F, int H, int W, double near, int iters, double reject,
                              double huber, double min_cos, int min_px, double tolerance, double pivot_min, void* workspace,
                              size_t workspace_bytes, double* RT, int32_t* status, int32_t* iters_out, double* err, int32_t* pairs,
                              void* stream);

/* ---------------------------------------------------------------------------------------
 * Training frames from meshes: colour, depth, instance mask, face ids and per-slot visibility statistics of n frames of S posed
 * objects each (render.render_frames_numpy restates the rule bit for bit).  Parity with BOP's renderers or with
 * BlenderProc's PBR frames is NOT claimed: the image is defined by the rule written here.
 *
 * THE SCENE  O meshes concatenated: verts f32[Vt,3] (verts_f64 0) or f64[Vt,3] (1), vcol u8[Vt,3], vnrm f32[Vt,3] (object frame);
 * faces i32[Ft,3] index the concatenated vertices; obj_face0: HOST array i32[O+1], object o owns the faces obj_face0[o] ..
 * obj_face0[o+1]-1 (strictly ascending, from >= 0 to <= Ft; refused otherwise).  slot_obj i32[n,S]: the object of each slot, -1 for
 * an empty one -- DEVICE data the entry cannot look at: the kernel treats every value outside [0, O) as an empty slot and never
 * indexes with it.  RT f64[n,S,3,4]; K f64[3,3] (k_per_instance 0) or f64[n,3,3] (1); light f64[n,3], a unit vector in the camera
 * frame pointing from the surface towards the light; ambient in [0, 1]; near >= 0.
 *
 * THE RULE  Coverage and depth of every triangle are THE PIXEL RULE of gdm_render_depth_hip above, unchanged (one copy of the code
 * serves both entries).
 *   layers      per (frame, slot, pixel) the minimum over the object's covering faces of the 64-bit key (fp32 depth bits << 32) |
 *               global face id: the nearest face, the lower id among equal depths.  Order-independent, hence reproducible.
 *   winner      per pixel the slot with the smallest depth bits, the lower slot on a tie
 *   attributes  the winning face is set up again; when the winding normalisation swapped vertices 1 and 2 their attributes swap too.
 *               With w_i the edge values at the pixel: q_i = (double) w_i * (1 / z_i), Q = (q0 + q1) + q2, and every attribute is
 *               ((q0 a0 + q1 a1) + q2 a2) / Q in fp64 -- the colour channels as levels 0..255, the normal's three components
 *   shading     the interpolated normal o is rotated by the slot's R, n_i = (R_i0 ox + R_i1 oy) + R_i2 oz;
 *               len = sqrt((nx nx + ny ny) + nz nz); cos = len > 0 ? max(((nx lx + ny ly) + nz lz) / len, 0) : 0;
 *               k = ambient + (1 - ambient) cos; channel = (u8) min(255, floor(c k + 0.5))
 * OUTPUTS  rgb u8[n,H,W,3]; depth f32[n,H,W] (the winner's, 0 where empty); inst u8[n,H,W] (slot + 1, 0 where empty); face
 * i32[n,H,W] (-1 where empty); stats i32[n,S,6] = (px_all, px_vis, xmin, ymin, xmax, ymax): px_all = the non-empty pixels of the
 * slot's own layer (BOP's px_count_all, clipped to the image), px_vis = the pixels the slot wins, the box that of the won pixels,
 * (W, H, -1, -1) when there are none.
 * workspace: gdm_render_frames_workspace_bytes(n, S, H, W) = n S H W 8 bytes (the layers; 0 for arguments the entry refuses),
 * 8-byte aligned.  No allocation and no host read: the call captures in a hipGraph.
 * LIMITS (what the index arithmetic addresses; refused beyond): S <= GDM_RENDER_MAX_SLOTS, O <= GDM_RENDER_MAX_OBJECTS (the face
 * ranges travel by value in the kernel arguments), n <= 65535, H, W <= 16384, n S Fmax <= 2^30 with Fmax the largest object's face
 * count. */
enum { GDM_RENDER_MAX_SLOTS = 8, GDM_RENDER_MAX_OBJECTS = 256 };
size_t gdm_render_frames_workspace_bytes(int n, int S, int H, int W);
int gdm_render_frames_hip(const void* verts, int verts_f64, const uint8_t* vcol, const float* vnrm, const int32_t* faces,
                          const int32_t* obj_face0 /* host array */, const int32_t* slot_obj, const double* RT, const double* K,
                          int k_per_instance, const double* light, double ambient, double near, int n, int S, int O, int Vt, int Ft,
                          int H, int W, void* workspace, size_t workspace_bytes, uint8_t* rgb, float* depth, uint8_t* inst,
                          int32_t* face, int32_t* stats, void* stream);

/* ---------------------------------------------------------------------------------------
 * Textures: the appearance of a mesh that carries (u, v) per face corner and an image instead of vertex colours (BOP's YCB-V, HB,
 * TUD-L models; texture.py restates the rule in numpy bit for bit).  Parity with BOP's GL renderers is NOT claimed: the
 * level choice is isotropic, one level per pixel without a trilinear blend, and blurs at grazing angles.
 *
 * THE TEXTURE RULE
 *   storage   an object's texture is a pyramid of texels u8[T,4] = (r, g, b, 0), one dword each.  Level 0 is the image, W0 x H0, row
 *             major, row 0 the image's top row; level l has W_l x H_l = max(1, W0 >> l) x max(1, H0 >> l) texels and follows level
 *             l - 1 without a gap; 1 <= L <= 1 + floor(log2(max(W0, H0))) levels.  All objects' pyramids lie in one buffer of
 *             tex_texels texels, 1 <= tex_texels < 2^31, 4-byte aligned.
 *   table     tex_tab i64[O,4] = (offset in texels, W0, H0, L) per object; W0 = 0: no texture, the vertex colours.  DEVICE data the
 *             entry cannot look at: a kernel uses a row only when W0, H0 in [1, 16384], L in [1, 1 + floor(log2(max(W0, H0)))],
 *             offset >= 0 and offset + (the texels of the L levels) <= tex_texels; every other row counts as "no texture", and no
 *             address outside the buffer is ever formed.
 *   mips      texel (x, y) of level l = per channel (a + b + c + d + 2) >> 2 over the texels (2x, 2y), (2x+1, 2y), (2x, 2y+1),
 *             (2x+1, 2y+1) of level l - 1, each index clamped to that level.
 *   fetch     Fetch(l, u, v), fp64: x = u W_l - 0.5, y = (flip_v ? 1 - v : v) H_l - 0.5 (flip_v = 1, the default of a definition,
 *             makes v = 0 the image's bottom row); x0 = floor(x), fx = (int) floor((x - x0) 256), likewise y0, fy; the texels
 *             c00 = (x0, y0), c10 = (x0 + 1, y0), c01 = (x0, y0 + 1), c11 = (x0 + 1, y0 + 1) with every index clamped to the level
 *             (clamp to edge); per channel ((c00 (256 - fx) + c10 fx) (256 - fy) + (c01 (256 - fx) + c11 fx) fy + 32768) >> 16.
 *             A u or v that is not finite fetches texel (0, 0) of the level.
 *   level     no transcendental.  With (U, V) = (u W0, v H0) at the pixel and at its neighbours (px + 1, py) and (px, py + 1):
 *             dUx = Ux - U, dVx = Vx - V, dUy, dVy likewise; a = dUx dUx + dVx dVx, b = dUy dUy + dVy dVy; rho2 = the larger of a
 *             and b, NaN when either is; the level is the smallest l with rho2 <= 4^l, capped at L - 1 (a NaN ends there too).
 *
 * gdm_texture_pyramid_texels(H, W, L): the texels of the L levels of an H x W image; 0 for what gdm_texture_mips_hip refuses.
 * gdm_texture_mips_hip: image u8[H,W,3] -> pyr, pyr_texels >= gdm_texture_pyramid_texels(H, W, L) texels (4-byte aligned, below
 * 2^31): level 0 packed, levels 1 .. L-1 built, one launch per level.  No memset node, no allocation, no host read. */
long gdm_texture_pyramid_texels(int H, int W, int L);
int gdm_texture_mips_hip(const uint8_t* image, int H, int W, int L, void* pyr, long pyr_texels, void* stream);
/* gdm_render_frames_tex_hip: gdm_render_frames_hip with textures.  fuv f32[Ft,3,2]: a (u, v) for every corner of every face of the
 * scene (those of untextured objects are not read); tex, tex_tab, tex_texels as above, one row per object of obj_face0; flip_v 0 or 1.
 * The clear and visibility passes are those of gdm_render_frames_hip; so is everything the resolve pass writes but rgb at the pixels
 * whose winning slot holds an object with a valid table row.  There:
 *   corners     the face's three (u, v) in stored order; when the winding normalisation swapped vertices 1 and 2, corners 1 and 2 swap
 *   uv          u and v by ((q0 a0 + q1 a1) + q2 a2) / Q, fp64, like every attribute
 *   neighbours  the same with the face's edge values at (px + 1, py) and at (px, py + 1), whether or not the face covers them;
 *               a neighbour whose Q is not > 0 sends the pixel to level L - 1
 *   colour      c = Fetch(level, u, v) by THE TEXTURE RULE, then the shading of gdm_render_frames_hip per channel:
 *               (u8) min(255, floor(c k + 0.5))
 * A slot whose object has no valid row is coloured from vcol, bit for bit as gdm_render_frames_hip does; with no valid row at all
 * the two entries write the same bytes.  Captures in a hipGraph. */
int gdm_render_frames_tex_hip(const void* verts, int verts_f64, const uint8_t* vcol, const float* vnrm, const int32_t* faces,
                              const int32_t* obj_face0 /* host array */, const int32_t* slot_obj, const double* RT, const double* K,
                              int k_per_instance, const double* light, double ambient, double near, int n, int S, int O, int Vt, int Ft,
                              int H, int W, void* workspace, size_t workspace_bytes, uint8_t* rgb, float* depth, uint8_t* inst,
                              int32_t* face, int32_t* stats, const float* fuv, const void* tex, const int64_t* tex_tab, long tex_texels,
                              int flip_v, void* stream);

/* ---------------------------------------------------------------------------------------
 * A structured-light depth sensor on a metric depth frame (sensor.simulate_depth_sensor_numpy restates the rule and
 * the kernel equals it bit for bit).  A function of the depth frame alone: what gdm_render_frames_hip or gdm_render_depth_hip drew,
 * or any other depth in metres.  Parity with a real device, with BlenSor or with simkinect is NOT claimed: the rule is the definition.
 *
 * INPUTS  depth f32[n,H,W] in metres (0, negative or NaN: no depth);  K: a HOST array f32[n,3,3] (k_per_frame 1) or f32[3,3]
 * (k_per_frame 0), fx = K[0], cx = K[2], fy = K[4], cy = K[5] -- host data, because the shadow window below is checked before the
 * launch; the intrinsics travel by value in the kernel arguments, so k_per_frame 1 wants n <= GDM_SENSOR_MAX_K;  baseline (metres,
 * signed and not 0: the projector sits at camera x = +baseline), z_min, z_max, sigma_d (pixels of disparity), subpixel (disparity
 * steps per pixel), cos_min <= cos_soft, p_shift;  stages: the sum of GDM_SENSOR_RANGE 1, GDM_SENSOR_SHADOW 2, GDM_SENSOR_GRAZING 4,
 * GDM_SENSOR_JITTER 8, GDM_SENSOR_NOISE 16 -- a stage whose bit is clear is skipped;  seed, and seed_dev as for
 * gdm_sample_assemble_hip.
 * OUTPUTS  out_depth f32[n,H,W], 0 where the sensor returns nothing;  cause u8[n,H,W]: 0 measured, 1 empty in the input, 2 out of
 * range, 3 projector shadow, 4 grazing, 5 jittered onto a pixel outside the frame.  Neither output may overlap the input.
 *
 * THE SENSOR RULE.  All arithmetic is fp32, one rounding per operation in the order written (the library is built with
 * -ffp-contract=off), but for fb.  No transcendental and no square root anywhere.  Pixel (x, y) of frame b, p = y W + x, z = depth.
 *   draws     mix = lowbias32 as above;  hb = mix(mix(seed ^ 0x27d4eb2f) ^ b);  the pixel word of stream s is mix(mix(hb ^ s) ^ p),
 *             s = 1 grazing, 2 jitter, 3 noise
 *   fb        (float) ((double) fx (double) |baseline|): fp64, rounded once;  D(z) = fb / z, the disparity in pixels
 *   valid     z > 0 (false for NaN); otherwise cause 1
 *   1 range   a valid pixel with !(z >= z_min && z <= z_max) gets cause 2.  The pixels that are valid and not dropped here SURVIVE;
 *             with the stage off every valid pixel survives.  A pixel out of range casts no shadow and is no neighbour in stage 3
 *             either: a simplification -- a real surface nearer than z_min still blocks the projector.
 *   2 shadow  Wd = (int) ceilf(fb / z_min), the widest disparity a survivor can have.
 *             baseline > 0:  g(x) = (float) x - D;  a survivor x is shadowed (cause 3) iff some survivor x' of its row has
 *                            0 < x' - x <= Wd and g(x') <= g(x)
 *             baseline < 0:  g(x) = (float) x + D;  shadowed iff some survivor x' of its row has 0 < x - x' <= Wd and g(x') >= g(x)
 *             (the shadow lies left of an occluder for a positive baseline, right of it for a negative one, and is D_near - D_far
 *             wide).  A windowed minimum of identical fp32 values: any scan order gives the same bits.  A shadowed pixel still casts.
 *   3 grazing for a survivor that stage 2 kept:  P(x, y) = (z u, z v, z) with u = ((float) x - cx) / fx, v = ((float) y - cy) / fy.
 *             tx = P(x+1, y) - P(x-1, y) when both neighbours survive, else P(x+1, y) - P(x, y), else P(x, y) - P(x-1, y), by which
 *             neighbour survives (a pixel outside the frame does not); ty likewise with y.  No tangent in a direction: cause 4.
 *             nrm = tx x ty, each component a b - c d as two products and one subtraction, in the order
 *             (tx.y ty.z - tx.z ty.y, tx.z ty.x - tx.x ty.z, tx.x ty.y - tx.y ty.x);  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z;
 *             c2 = (dot(nrm, P) dot(nrm, P)) / (dot(nrm, nrm) dot(P, P))   (the squared cosine of the incidence angle)
 *             cmin2 = cos_min cos_min, csoft2 = cos_soft cos_soft.  !(c2 >= cmin2): cause 4 (a NaN c2 too).  Otherwise, when
 *             c2 < csoft2:  r = (csoft2 - c2) / (csoft2 - cmin2);  T = (uint32) (r 16777216.0f) (truncated, 0 .. 2^24);
 *             cause 4 iff (word of stream 1 >> 8) < T.  At a silhouette the difference runs across the depth step, so the rim
 *             frays: intended.
 *   4 jitter  T = (uint32) (p_shift 32768.0f);  w = the word of stream 2;  for h = w & 0xffff: jx = h < T ? -1 : (h >= 65536 - T ?
 *             1 : 0);  jy the same from h = w >> 16.  Output pixel p reads source pixel q = (x + jx, y + jy); with the stage off
 *             q = p.  q outside the frame: cause 5.  q with a cause from stages 1 - 3 (or empty): p takes that cause.
 *   5 noise   zeta = (sum of the four bytes of the word of stream 3 at p) - 510 (Irwin-Hall, as in the augmentation rule);
 *             e = (float) zeta 0.0067658751f (= 1 / sqrt(21845): unit variance);  D' = D(z(q)) + sigma_d e;
 *             Dq = rintf(D' subpixel) / subpixel;  !(Dq > 0): cause 2;  otherwise out = fb / Dq, cause 0.
 *             With the stage off out = z(q), the input's bits.
 * THE CALL  one launch whatever n, one workgroup per (frame, GDM_SENSOR_TILE_W x GDM_SENSOR_TILE_H tile).  The tile keeps its pixels'
 * surviving depth with a ring of 2 (stage 4 reads stage-3 results one pixel away, which read stage-1 depth one pixel further) and Wd
 * further columns on the projector side in LDS, recomputes the halo, and takes the windowed minimum by log-step doubling in LDS
 * (ceil(log2 Wd) passes, not Wd steps per pixel).  No workspace, no atomics, no allocation, no host read: it captures in a hipGraph
 * and redraws from seed_dev on replay.
 * LIMITS (refused beyond, before any HIP call): 1 <= n <= 65535, 1 <= H, W <= 16384; finite fx, fy > 0; baseline finite, not 0;
 * z_min > 0, z_max > z_min; sigma_d >= 0; subpixel >= 1; 0 <= cos_min <= cos_soft <= 1; 0 <= p_shift <= 1; stages in [0, 31];
 * 1 <= Wd <= GDM_SENSOR_MAX_DISP for every frame (checked whether or not stage 2 is on). */
enum { GDM_SENSOR_RANGE = 1, GDM_SENSOR_SHADOW = 2, GDM_SENSOR_GRAZING = 4, GDM_SENSOR_JITTER = 8, GDM_SENSOR_NOISE = 16 };
enum { GDM_SENSOR_MAX_DISP = 255, GDM_SENSOR_TILE_W = 128, GDM_SENSOR_TILE_H = 8, GDM_SENSOR_MAX_K = 64 };
int gdm_depth_sensor_hip(const float* depth, const float* K /* host array */, int k_per_frame, int n, int H, int W, float baseline,
                         float z_min, float z_max, float sigma_d, float subpixel, float cos_min, float cos_soft, float p_shift,
                         int stages, uint32_t seed, const uint32_t* seed_dev, float* out_depth, uint8_t* cause, void* stream);

/* ---------------------------------------------------------------------------------------
 * Object model preparation: from a triangle mesh to the table obj_%06d_fps.npy holds ([M,9] = xyz in mm, rgb 0..255, unit normal,
 * rows in farthest-point order; read by datasets/lm/linemod_pbr.py:89-97, evaluator.py:34-40, models/SplineCNN.py:116).  The script
 * that wrote the reference's files is not part of it, so each entry is defined by the rule written here, which model_prep.py
 * restates in numpy (surface_sample_numpy, fps_numpy, point_diameter_numpy) bit for bit; DESIGN.md 6n.  All fp32 arithmetic below
 * is single operations rounded to nearest, never fused, the division and the square root included.
 *
 * gdm_surface_sample_hip: S points on the mesh, faces drawn in proportion to integer weights, attributes interpolated.
 * verts, vnrm, vrgb f32[V,3] (vrgb holds integer levels 0..255); faces i32[F,3], every index in [0, V) (the CALLER checks that);
 * cdf i64[F] = the inclusive cumulative sum of non-negative integer face weights with cdf[F-1] > 0 (the caller checks that too: it
 * cannot be seen from the host here); out f32[S,9] = xyz, rgb, normal.  THE SAMPLE RULE for sample s, all words uint32:
 *   words     base = mix32(mix32(seed ^ 0x9e3779b9) ^ s), h_j = mix32(base ^ ((j + 1) * 0x9e3779b9 mod 2^32)) for j = 0..3, mix32 the
 *             lowbias32 of gdm_sample_assemble_hip
 *   face      target = floor(((h_0 << 32 | h_1) * cdf[F-1]) / 2^64) (__umul64hi); f = the first face with cdf[f] > target -- a face
 *             of weight 0 is never drawn
 *   weights   ui = h_2 >> 8, vi = h_3 >> 8; when ui + vi > 2^24 (u + v > 1, decided on the integers): ui = 2^24 - ui, vi = 2^24 - vi;
 *             u = ui * 2^-24, v = vi * 2^-24, w0 = (1 - u) - v -- all three exact and >= 0
 *   channels  x = ((w0 * A) + (u * B)) + (v * C) for each of the nine, A, B, C the values at the face's three vertices in its order
 *   colour    min(max(floor(x + 0.5), 0), 255)
 *   normal    l = sqrt(((nx * nx) + (ny * ny)) + (nz * nz)); each component divided by l when l > 0, a zero normal stays zero
 * One thread per sample, no atomics: the result does not depend on the launch shape.  1 <= S < 2^31, V >= 1, F >= 1. */
int gdm_surface_sample_hip(const float* verts, const int32_t* faces, const float* vnrm, const float* vrgb, const int64_t* cdf,
                           int V, int F, long S, uint32_t seed, float* out, void* stream);
/* gdm_surface_sample_tex_hip: gdm_surface_sample_hip for a textured mesh.  fuv f32[F,3,2] (a (u, v) per face corner), tex and
 * tex_texels as for gdm_render_frames_tex_hip, the object's table row BY VALUE (tex_off, tex_w, tex_h, tex_levels) and flip_v.  The
 * row is host data here: one that THE TEXTURE RULE calls invalid is refused, and tex_w = 0 (no texture) gives gdm_surface_sample_hip's
 * output.  Otherwise the same draws, and xyz and normal bit-equal to gdm_surface_sample_hip's for the same seed;
 *   colour    tu = ((w0 * u_A) + (u * u_B)) + (v * u_C), tv likewise, fp32 single operations like every channel; rgb = the three
 *             integers of Fetch(0, (double) tu, (double) tv): level 0, the samples are not pixels and have no footprint. */
int gdm_surface_sample_tex_hip(const float* verts, const int32_t* faces, const float* vnrm, const float* vrgb, const int64_t* cdf,
                               const float* fuv, const void* tex, int64_t tex_off, int64_t tex_w, int64_t tex_h, int64_t tex_levels,
                               long tex_texels, int flip_v, int V, int F, long S, uint32_t seed, float* out, void* stream);
/* gdm_fps_wide_hip: furthest point sampling for many candidates, spread over the whole device.  idx i32[B,m] equals what
 * gdm_furthestsampling_hip returns for the same xyz f32[B,n,3], bit for bit.  THE RULE both follow: pick 0 is index 0; dist starts
 * at 1e10; after pick p every candidate takes dist = fminf(dist, d2), d2 = ((dx * dx) + (dy * dy)) + (dz * dz) to p; the next pick
 * is the candidate of largest dist, the lowest index among equals.
 * The entry enqueues m launches of one small kernel and returns without synchronising.  In launch i (1..m) every workgroup reduces
 * the `groups` partial results launch i-1 left -- a partial is (float bits of dist) << 32 | (0xffffffff - index), so the unsigned
 * 64-bit maximum is the largest dist and then the lowest index; a workgroup with an empty slice leaves 0 --, takes the winner as
 * pick i-1 (workgroup 0 stores idx[i-1]; launch 1 reads nothing and takes index 0), updates dist over its own slice of
 * ceil(n / groups) candidates and writes its partial into half (i & 1) of partial.  Launch m only stores the last pick.  No workgroup
 * waits for another inside a kernel (no cooperative launch, no grid barrier, no flag): the order comes from the stream alone.
 * dist f32[B,n] is scratch (initialised inside, left unwritten when m == 1); partial: [B, 2, groups] 64-bit words, 8-byte aligned,
 * scratch.  groups: 1..1024, or 0 = gdm_fps_wide_groups(n) (one workgroup per 1024 candidates, at most 1024), which then sizes
 * partial.  B <= 65535, 1 <= m <= n. */
int gdm_fps_wide_groups(int n);
int gdm_fps_wide_hip(int B, int n, int m, int groups, const float* xyz, float* dist, void* partial, int32_t* idx, void* stream);
/* gdm_point_diameter_hip: the exact farthest pair of xyz f32[V,3]: pair i32[2] = the (i < j) of the largest
 * d2 = ((dx * dx) + (dy * dy)) + (dz * dz), the lowest i and then the lowest j among equals; d2 f32[1] is that value.  Row tiles of
 * 256 points in registers against column tiles in LDS over the upper triangle; every workgroup writes one packed partial into
 * workspace (gdm_point_diameter_workspace_bytes(V) bytes, 8-byte aligned; 0 for an unsupported V) and a second launch reduces
 * them.  No atomics: every run gives the same answer.  2 <= V <= 2^24. */
size_t gdm_point_diameter_workspace_bytes(int V);
int gdm_point_diameter_hip(const float* xyz, int V, int64_t* workspace, size_t workspace_bytes, int32_t* pair, float* d2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDM_H */
