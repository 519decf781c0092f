// Front end on the device, gfx950: the N points of every crop drawn by the counter-based rule of include/gdm.h
// (gdm_sample_assemble_hip) and the assembled item (choose, cld_rgb_nrm, labels, n_valid) from ONE launch -- what the loader does
// with np.random.shuffle / np.pad(..., 'wrap') and fancy indexing (datasets/lm/linemod_pbr.py:476-513).
//   sample_assemble_kernel   one workgroup of 1024 threads per crop; the keys are recomputed from the pixel index in every pass:
//     1. the valid map is read once: every wave turns 64 consecutive pixels into one 64-bit word of the crop's bitmap (workspace,
//        P / 8 bytes, read back by the same wave in later passes; a wave's first 64 words stay in its registers), the words'
//        popcounts add up to n_valid, and the top byte of every valid key goes into a 256-bin integer histogram in LDS;
//     2. with n_valid > N, a radix select of the N-th smallest key, 8 bits a step from the top: the bin that holds the rank fixes
//        the next byte of the threshold's prefix.  It stops as soon as that bin's keys fit the candidate list in LDS (at once for a
//        256 x 256 crop: 256 keys per bin); until then one more histogram pass over the bitmap per byte;
//     3. one pass compacts the (key, pixel) pairs into LDS: keys below the prefix are selected, keys on it are candidates; the
//        candidates are sorted and the lowest `rank` of them complete the selection -- exactly min(N, n_valid) pairs, the keys of a
//        crop being distinct; the pairs are padded to a power of two and sorted by a bitonic network;
//     4. point j takes pair j mod n: choose, the nine gathers of cld_rgb_nrm and the label.
// The result is fixed by the definition whatever order the LDS atomics land in.  No global atomics, no allocation, no host read: the
// launch captures in a hipGraph, and with seed_dev a replay draws from the word that pointer holds at that time.
#include "gdm_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kBatch = 8;                                                  // valid-map loads a lane keeps in flight
constexpr unsigned kCand = 2048;                                           // candidate pairs the select may leave to a sort in LDS

// lowbias32: the mixer of the RANSAC sampler (gdm_pose_robust.hip mix32, include/gdm.h), repeated here bit for bit.
__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// Ascending bitonic sort of a[0 .. n2), n2 a power of two, by the whole workgroup; ends with a barrier.
__device__ __forceinline__ void bitonic_sort(unsigned long long* a, unsigned n2, unsigned t)
{
    for (unsigned k = 2; k <= n2; k <<= 1) {
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned i = t; i < n2; i += kThreads) {
                const unsigned x = i ^ j;
                if (x > i) {
                    const unsigned long long u = a[i], v = a[x];
                    if ((u > v) == ((i & k) == 0)) { a[i] = v; a[x] = u; }
                }
            }
            __syncthreads();
        }
    }
}

// Word w of the crop's bitmap, for the wave that owns it: its first 64 words are in `kept` (word i in lane i), the rest in memory.
__device__ __forceinline__ unsigned long long bitmap_word(const unsigned long long* bitmap, unsigned long long kept, int w, int wave)
{
    const int i = (w - wave) / kWaves;                                     // uniform in the wave
    return i < 64 ? __shfl(kept, i, 64) : bitmap[w];
}

// Appends (key, pix) of the lanes with `sel` to list[*count ...): one LDS atomic per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void wave_append(bool sel, uint32_t key, uint32_t pix, unsigned long long* list, unsigned* count, unsigned cap,
                                            int lane)
{
    const unsigned long long sm = __ballot(sel);
    if (sm) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(count, (unsigned)__popcll(sm));
        base = __shfl(base, 0, 64);
        const unsigned at = base + (unsigned)__popcll(sm & ((1ull << lane) - 1ull));
        if (sel && at < cap) list[at] = ((unsigned long long)key << 32) | pix;      // at < cap by the counts of the select
    }
}

__global__ __launch_bounds__(kThreads) void sample_assemble_kernel(
    const float* __restrict__ valid_depth, const float* __restrict__ dpt_xyz, const float* __restrict__ rgb,
    const float* __restrict__ normals, const uint8_t* __restrict__ mask, int P, int N, uint32_t seed,
    const uint32_t* __restrict__ seed_dev, int32_t* __restrict__ choose, float* __restrict__ cld_rgb_nrm, uint8_t* __restrict__ labels,
    int32_t* __restrict__ n_valid_out, unsigned long long* __restrict__ bitmap_ws)
{
    __shared__ unsigned long long pairs[GDM_SAMPLE_MAX_N];                 // (key << 32) | pixel, 32 KB
    __shared__ unsigned long long cand[kCand];                             // 16 KB
    __shared__ unsigned hist[256];
    __shared__ unsigned wave_count[kWaves];
    __shared__ unsigned sel_prefix, sel_rank, sel_bin, n_pairs, n_cand;

    const int b = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int words = (P + 63) >> 6;
    unsigned long long* bitmap = bitmap_ws + (long)b * words;
    const float* vd = valid_depth + (long)b * P;
    const uint32_t hb = mix32(mix32((seed_dev ? *seed_dev : seed) ^ 0x9e3779b9u) ^ (uint32_t)b);

    // 1. bitmap, n_valid and the histogram of the keys' top byte.  Word w belongs to wave w % kWaves here and in every later pass.
    if (t < 256) hist[t] = 0;
    if (t == 0) { n_pairs = 0; n_cand = 0; }
    __syncthreads();
    //    The wave's first 64 words also stay in registers, word i in lane i: a 256 x 256 crop never reads the bitmap back.
    unsigned cnt = 0;
    unsigned long long kept = 0;
    for (int w0 = wave; w0 < words; w0 += kWaves * kBatch) {
        float d[kBatch];                                                   // kBatch independent loads in flight
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int w = w0 + u * kWaves, p = w * 64 + lane;
            d[u] = w < words && p < P ? vd[p] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int w = w0 + u * kWaves;
            if (w < words) {                                               // uniform in the wave
                const bool v = d[u] > 1e-6f;                               // NaN and negative depth compare false
                const unsigned long long m = __ballot(v);
                if (lane == 0) bitmap[w] = m;
                if (lane == (w - wave) / kWaves) kept = m;
                cnt += (unsigned)__popcll(m);                              // the same in every lane
                if (v) atomicAdd(&hist[mix32(hb ^ (uint32_t)(w * 64 + lane)) >> 24], 1u);
            }
        }
    }
    if (lane == 0) wave_count[wave] = cnt;
    __threadfence_block();
    __syncthreads();
    unsigned n_valid = 0;
    for (int i = 0; i < kWaves; ++i) n_valid += wave_count[i];
    if (t == 0) n_valid_out[b] = (int)n_valid;
    const unsigned n = n_valid < (unsigned)N ? n_valid : (unsigned)N;      // pairs to select

    // 2. the prefix of the n-th smallest key (rank n, counted from 1): keys below it are selected, and so are the lowest `rank` of
    //    the keys on it.  Without a selection (n_valid <= N) rank stays 0 and every valid key is selected.
    uint32_t prefix = 0, pmask = 0;
    unsigned rank = 0;
    if (n_valid > (unsigned)N) {
        rank = n;
        for (int shift = 24; ; shift -= 8) {
            if (shift != 24) {                                             // the histogram of the next byte among the keys on the prefix
                if (t < 256) hist[t] = 0;
                __syncthreads();
                for (int w = wave; w < words; w += kWaves) {
                    const unsigned long long m = bitmap_word(bitmap, kept, w, wave);
                    if ((m >> lane) & 1ull) {
                        const uint32_t key = mix32(hb ^ (uint32_t)(w * 64 + lane));
                        if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
                    }
                }
                __syncthreads();
            }
            if (wave == 0) {                                               // the bin that holds the rank: lane l scans bins 4l .. 4l+3
                const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
                const unsigned s = h0 + h1 + h2 + h3;
                unsigned incl = s;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned o = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += o;
                }
                const unsigned excl = incl - s, k = rank;
                if (excl < k && k <= incl) {                               // exactly one lane: the counts sum to at least k
                    unsigned r = k - excl, digit = 4 * lane, c = h0;
                    if (r > h0) { r -= h0; ++digit; c = h1; if (r > h1) { r -= h1; ++digit; c = h2; if (r > h2) { r -= h2; ++digit; c = h3; } } }
                    sel_prefix = prefix | (digit << shift);
                    sel_rank = r;
                    sel_bin = c;
                }
            }
            __syncthreads();
            prefix = sel_prefix;
            pmask |= 0xffu << shift;
            rank = sel_rank;
            const unsigned bin = sel_bin;                                  // (written again only behind the next pass's barriers)
            if (bin <= kCand || shift == 0) break;                         // at shift 0 the prefix is the key itself: one candidate
        }
    }

    // 3. compaction: keys below the prefix into the pairs, keys on it into the candidates; the lowest `rank` candidates follow
    const bool all = rank == 0;                                            // the select leaves rank >= 1
    for (int w = wave; w < words; w += kWaves) {
        const unsigned long long m = bitmap_word(bitmap, kept, w, wave);
        const uint32_t pix = (uint32_t)(w * 64 + lane);
        const uint32_t key = mix32(hb ^ pix);
        const bool v = (m >> lane) & 1ull;
        const uint32_t top = key & pmask;
        wave_append(v && (all || top < prefix), key, pix, pairs, &n_pairs, GDM_SAMPLE_MAX_N, lane);
        wave_append(v && !all && top == prefix, key, pix, cand, &n_cand, kCand, lane);
    }
    __syncthreads();
    if (!all) {
        const unsigned nc = n_cand < kCand ? n_cand : kCand;
        unsigned c2 = 1;
        while (c2 < nc) c2 <<= 1;
        for (unsigned i = nc + t; i < c2; i += kThreads) cand[i] = ~0ull;
        __syncthreads();
        bitonic_sort(cand, c2, t);
        const unsigned take = rank < n ? rank : n;                        // rank <= n by the select
        for (unsigned i = t; i < take; i += kThreads) pairs[n - take + i] = cand[i];
    }
    unsigned n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (unsigned i = n + t; i < n2; i += kThreads) pairs[i] = ~0ull;
    __syncthreads();
    bitonic_sort(pairs, n2, t);

    // 4. write-out: point j is pair j mod n (wrap-around padding); no valid pixel -> pixel 0
    const float* xyz_b = dpt_xyz + (long)b * P * 3;
    const float* rgb_b = rgb + (long)b * 3 * P;
    const float* nrm_b = normals + (long)b * 3 * P;
    float* out_b = cld_rgb_nrm + (long)b * 9 * N;
    for (int j = t; j < N; j += kThreads) {
        const uint32_t pix = n ? (uint32_t)(pairs[(unsigned)j % n] & 0xffffffffull) : 0u;
        choose[(long)b * N + j] = (int32_t)pix;
        const float* x = xyz_b + (long)pix * 3;
        out_b[j] = x[0]; out_b[N + j] = x[1]; out_b[2 * N + j] = x[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            out_b[(3 + c) * N + j] = rgb_b[(long)c * P + pix];
            out_b[(6 + c) * N + j] = nrm_b[(long)c * P + pix];
        }
        if (labels) {
            const uint8_t l = mask[(long)b * P + pix];
            labels[(long)b * N + j] = l == 255 ? (uint8_t)1 : l;
        }
    }
}

} // namespace

extern "C" size_t gdm_sample_assemble_workspace_bytes(int B, int S)
{
    if (B < 1 || B > 65535 || S < 1 || S > GDM_SAMPLE_MAX_S) return 0;
    return (size_t)B * (size_t)(((long)S * S + 63) / 64) * 8;
}

extern "C" int gdm_sample_assemble_hip(const float* valid_depth, const float* dpt_xyz, const float* rgb, const float* normals,
                                       const uint8_t* mask, int B, int S, int N, uint32_t seed, const uint32_t* seed_dev, int32_t* choose,
                                       float* cld_rgb_nrm, uint8_t* labels, int32_t* n_valid, void* workspace, size_t workspace_bytes,
                                       void* stream)
{
    GDM_CHECK_ARG(valid_depth && dpt_xyz && rgb && normals && choose && cld_rgb_nrm && n_valid && workspace,
                  "gdm_sample_assemble_hip: NULL pointer");
    GDM_CHECK_ARG((mask == nullptr) == (labels == nullptr), "gdm_sample_assemble_hip: mask and labels go together (both or neither)");
    GDM_CHECK_ARG(B >= 1 && B <= 65535, "gdm_sample_assemble_hip: B=%d not in [1, 65535]", B);
    GDM_CHECK_ARG(S >= 1 && S <= GDM_SAMPLE_MAX_S, "gdm_sample_assemble_hip: S=%d not in [1, %d]", S, GDM_SAMPLE_MAX_S);
    GDM_CHECK_ARG(N >= 1 && N <= GDM_SAMPLE_MAX_N, "gdm_sample_assemble_hip: N=%d not in [1, %d]", N, GDM_SAMPLE_MAX_N);
    const size_t need = gdm_sample_assemble_workspace_bytes(B, S);
    GDM_CHECK_ARG(workspace_bytes >= need, "gdm_sample_assemble_hip: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    GDM_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "gdm_sample_assemble_hip: workspace must be 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sample_assemble_kernel, dim3(B), dim3(kThreads), 0, s, valid_depth, dpt_xyz, rgb, normals, mask, S * S, N, seed,
                       seed_dev, choose, cld_rgb_nrm, labels, n_valid, (unsigned long long*)workspace);
    return gdm_launch_status("sample_assemble_kernel");
}
