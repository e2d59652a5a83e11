// CascadeROIHeads in training (afigan_amd/roi_heads.py): the two passes that are specific to this package's padded [N][B] row lists with
// device-side counts.
//   afi_roi_cascade_relabel   detectron2 v0.1.1's _create_proposals_from_boxes + _match_and_label_boxes: decode stage k's deltas with the very
//                             device function afi_roi_cascade_stage instantiates (afi_roi_decode.h), drop the boxes that clipped to empty keeping
//                             the order, match the survivors at the next stage's threshold (afi_box_match.h).  One 256-thread block per image:
//                             the image's ground truth sits in LDS, a chunk of 256 rows is decoded one row per thread, the kept flags are
//                             counted by a ballot per wave and a four-entry LDS exchange, and the block carries the running count from chunk
//                             to chunk -- a stable compaction without atomics, bit-identical between runs.
//   afi_roi_bn_*              train-mode BatchNorm + ReLU over x [N B][P1][C] in which only the rows j < counts[n] of image n exist.  The
//                             reductions walk LIST rows (a block takes a range of them, skips the padding rows without reading them, and its 8
//                             pixel lanes x 32 channel quads take the P1 pixels of a valid row with 16-byte loads); partials [chunks][2][C] are
//                             summed by 8 lanes per channel in a fixed order, as in elementwise.hip.  The statistics accumulate in fp64,
//                             shifted by the first valid pixel, and are rounded once.  The two apply passes give one list row to a block at a
//                             time: a padding row is written as zeros and never read.  Pn = P1 sum(min(counts, B)) is formed on the device.
// Nothing here synchronises with the host or uses atomics.
#include "../../include/afigan_hip.h"
#include "afi_common.h"
#include "afi_roi_decode.h"
#include "afi_box_match.h"
#include "afi_bn.h"

#define CT_MAX_K 1024
#define CT_MAX_GT 1024              // RPN_MAX_GT: the ground truth of an image, held in LDS (20 KiB)
#define CT_MAX_B 4096               // RPN_MAX_BATCH
#define CT_MAX_N 1024               // images per call of the afi_roi_bn_* passes: every thread walks the N counts once (ct_valid_rows), a few
                                    // scalar loads at a training batch; a longer list is refused, not walked
#define CT_RED_MAX_CHUNKS 256       // AFI_RED_MAX_CHUNKS: afi_reduce_scratch_floats(C) holds [256][2][C] fp64 partials + [2][C]
#define CT_FIN_CH 32
#define CT_EW_GRID_CAP 2048         // 256 CUs x 8 blocks

__device__ __forceinline__ int ct_clamp_count(int c, int hi) { return c < 0 ? 0 : (c > hi ? hi : c); }

// ------------------------------------------------------------------------------------------------ relabel
__global__ __launch_bounds__(256) void afi_roi_cascade_relabel_kernel(const RoiDecode d, const float* __restrict__ pred,
                                                                      const float* __restrict__ proposals, const int* __restrict__ counts,
                                                                      const float* __restrict__ image_hw, const float* __restrict__ gt,
                                                                      const int* __restrict__ gt_classes, const int* __restrict__ counts_g,
                                                                      int Gmax, float thresh, float* __restrict__ boxes,
                                                                      int* __restrict__ counts_out, int* __restrict__ classes,
                                                                      float* __restrict__ gt_boxes, int* __restrict__ src,
                                                                      int* __restrict__ matched_idx) {
    __shared__ float4 sb[CT_MAX_GT];
    __shared__ float sa[CT_MAX_GT];
    __shared__ int wtot[4];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, B = d.P, K = d.K;
    const int cnt = ct_clamp_count(counts[n], B), G = ct_clamp_count(counts_g[n], Gmax);
    for (int g = tid; g < G; g += 256) {
        const float* q = gt + ((long long)n * Gmax + g) * 4;
        const float4 b = make_float4(q[0], q[1], q[2], q[3]);
        sb[g] = b;
        sa[g] = afi_box_area(b);
    }
    __syncthreads();
    const float ih = image_hw[2 * n], iw = image_hw[2 * n + 1];
    const long long row0 = (long long)n * B;
    int base = 0;                                            // kept rows of the chunks before this one (the same in every thread)
    for (int j0 = 0; j0 < cnt; j0 += 256) {
        const int j = j0 + tid;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        bool keep = false;
        if (j < cnt) {
            const long long row = row0 + j;
            roi_decode_clip(d, pred + row * d.ld + K + 1, roi_box_geom(proposals + 4 * row), ih, iw, o);
            keep = (o[2] - o[0] > 0.f) && (o[3] - o[1] > 0.f);             // Boxes.nonempty() in fp32; false for a NaN box
        }
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        int off = base + before, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) off += wtot[w];
            tot += wtot[w];
        }
        if (keep) {
            const float4 c = make_float4(o[0], o[1], o[2], o[3]);
            const float carea = afi_box_area(c);
            AfiMatch m{0.f, 0};
            for (int g = 0; g < G; ++g) afi_match_update(m, afi_box_iou(sb[g], sa[g], c, carea), g);
            const int label = G > 0 ? afi_match_label(m.val, thresh, thresh) : 0;
            const long long r = row0 + off;
            *(float4*)(boxes + 4 * r) = c;
            *(float4*)(gt_boxes + 4 * r) = G > 0 ? sb[m.idx] : make_float4(0.f, 0.f, 0.f, 0.f);
            classes[r] = label == 1 ? gt_classes[(long long)n * Gmax + m.idx] : K;
            src[r] = j;
            matched_idx[r] = m.idx;
        }
        base += tot;
        __syncthreads();                                     // wtot is rewritten by the next chunk
    }
    for (int j = base + tid; j < B; j += 256) {
        const long long r = row0 + j;
        *(float4*)(boxes + 4 * r) = make_float4(0.f, 0.f, 0.f, 0.f);
        *(float4*)(gt_boxes + 4 * r) = make_float4(0.f, 0.f, 0.f, 0.f);
        classes[r] = -1;
        src[r] = -1;
        matched_idx[r] = 0;
    }
    if (tid == 0) counts_out[n] = base;
}

extern "C" int afi_roi_cascade_relabel(const float* pred, long long ld_pred, int N, int B, int K, const float* proposals, const int* counts,
                                       const float* image_hw, float wx, float wy, float ww, float wh, double scale_clamp, const float* gt,
                                       const int* gt_classes, const int* counts_g, int Gmax, float iou_thresh, float* boxes, int* counts_out,
                                       int* classes, float* gt_boxes, int* src, int* matched_idx, void* stream) {
    if (!pred || !proposals || !counts || !image_hw || !gt || !gt_classes || !counts_g || !boxes || !counts_out || !classes || !gt_boxes || !src ||
        !matched_idx || N <= 0 || N > 65535 || B <= 0 || K <= 0 || Gmax <= 0 || !(iou_thresh == iou_thresh))
        return AFI_ERR_BAD_ARG;
    if (K > CT_MAX_K || B > CT_MAX_B || Gmax > CT_MAX_GT) return AFI_ERR_UNSUPPORTED;
    if (ld_pred < (long long)K + 1 + 4) return AFI_ERR_BAD_ARG;
    if (!(wx > 0.f) || !(wy > 0.f) || !(ww > 0.f) || !(wh > 0.f)) return AFI_ERR_BAD_ARG;
    if (((uintptr_t)boxes & 15) || ((uintptr_t)gt_boxes & 15)) return AFI_ERR_UNSUPPORTED;
    const RoiDecode d{N, B, K, 1, ld_pred, wx, wy, ww, wh, scale_clamp};
    hipLaunchKernelGGL(afi_roi_cascade_relabel_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, d, pred, proposals, counts, image_hw,
                       gt, gt_classes, counts_g, Gmax, iou_thresh, boxes, counts_out, classes, gt_boxes, src, matched_idx);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ list-masked BatchNorm + ReLU
struct CtList { const int* counts; int N, B, P1, C; };

// Pn / P1: the valid list rows of the call, and (first) the first of them, -1 when there is none.  Uniform: every thread runs the same loop.
__device__ __forceinline__ long long ct_valid_rows(const CtList& L, int* first) {
    long long v = 0;
    int f = -1;
    for (int n = 0; n < L.N; ++n) {
        const int c = ct_clamp_count(L.counts[n], L.B);
        if (c > 0 && f < 0) f = n * L.B;
        v += c;
    }
    if (first) *first = f;
    return v;
}
__device__ __forceinline__ bool ct_row_valid(const CtList& L, int l) {
    const int n = l / L.B;
    return l - n * L.B < ct_clamp_count(L.counts[n], L.B);
}

// Block = 32 channel quads x 8 pixel lanes; grid = (C / 128, chunks); a chunk is rows_per_chunk LIST rows.
// STATS: partial (fp64) [chunks][2][C] = sum (x - k), sum (x - k)^2 with k the first valid pixel of the call.
typedef double ct_f64x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void afi_roi_bn_stats_partial_kernel(const float* __restrict__ x, const CtList L, int rows_per_chunk,
                                                                       double* __restrict__ partial) {
    __shared__ ct_f64x4 red[2][8][32];
    const int cq = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 128 + cq * 4, C = L.C, R = L.N * L.B;
    const bool cok = c < C;
    int first;
    (void)ct_valid_rows(L, &first);
    ct_f64x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    if (cok && first >= 0) {
        const f32x4 k = *(const f32x4*)(x + (long long)first * L.P1 * C + c);
        const int l0 = blockIdx.y * rows_per_chunk, l1 = l0 + rows_per_chunk < R ? l0 + rows_per_chunk : R;
        for (int l = l0; l < l1; ++l) {
            if (!ct_row_valid(L, l)) continue;
            const float* xr = x + (long long)l * L.P1 * C + c;
            for (int p = rl; p < L.P1; p += 8) {
                const f32x4 v = *(const f32x4*)(xr + (long long)p * C);
#pragma unroll
                for (int j = 0; j < 4; ++j) { const double dd = (double)v[j] - (double)k[j]; s0[j] += dd; s1[j] += dd * dd; }
            }
        }
    }
    red[0][rl][cq] = s0; red[1][rl][cq] = s1;
    __syncthreads();
    if (rl == 0 && cok) {
#pragma unroll
        for (int i = 1; i < 8; ++i) { s0 += red[0][i][cq]; s1 += red[1][i][cq]; }
        double* dst = partial + (long long)blockIdx.y * 2 * C;
        *(ct_f64x4*)(dst + c) = s0;
        *(ct_f64x4*)(dst + C + c) = s1;
    }
}

// 32 channels per block, 8 lanes per channel take every 8th chunk; the lanes meet through LDS in a fixed order.
__global__ __launch_bounds__(256) void afi_roi_bn_stats_finalize_kernel(const double* __restrict__ partial, int chunks, const float* __restrict__ x,
                                                                        const CtList L, float* __restrict__ mean, float* __restrict__ invstd,
                                                                        float* __restrict__ var_out, float* __restrict__ running_mean,
                                                                        float* __restrict__ running_var, long long* __restrict__ nbt, float eps,
                                                                        float momentum) {
    __shared__ double red[2][8][CT_FIN_CH];
    const int cl = threadIdx.x & (CT_FIN_CH - 1), ln = threadIdx.x / CT_FIN_CH, C = L.C;
    const int c = blockIdx.x * CT_FIN_CH + cl;
    int first;
    const long long Pn = ct_valid_rows(L, &first) * L.P1;
    if (nbt && Pn > 0 && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;            // torch BatchNorm2d in train mode
    double a0 = 0.0, a1 = 0.0;
    if (c < C)
        for (int i = ln; i < chunks; i += 8) { a0 += partial[(long long)i * 2 * C + c]; a1 += partial[(long long)i * 2 * C + C + c]; }
    red[0][ln][cl] = a0; red[1][ln][cl] = a1;
    __syncthreads();
    if (ln != 0 || c >= C) return;
    if (Pn == 0) {                                           // no valid row: the statistics of nothing, the running buffers untouched
        mean[c] = 0.f;
        invstd[c] = (float)(1.0 / sqrt((double)eps));
        if (var_out) var_out[c] = 0.f;
        return;
    }
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { s0 += red[0][j][cl]; s1 += red[1][j][cl]; }
    const double inv_n = 1.0 / (double)Pn;
    const double dm = s0 * inv_n;                            // mean - k
    const double m = (double)x[(long long)first * L.P1 * C + c] + dm;
    double var = s1 * inv_n - dm * dm;                       // biased
    var = var > 0.0 ? var : 0.0;
    mean[c] = (float)m;
    invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (var_out) var_out[c] = (float)var;
    if (running_mean) {
        const double unb = var * ((double)Pn / (double)(Pn > 1 ? Pn - 1 : 1));
        running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * m);
        running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unb);
    }
}

// partial (fp32) [chunks][2][C] = sum g', sum g' xhat over the valid rows of the chunk; g' = g [y > 0] (RELU) from the stored y.
template <bool RELU>
__global__ __launch_bounds__(256) void afi_roi_bn_bwd_partial_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                     const float* __restrict__ y, const CtList L,
                                                                     const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                     int rows_per_chunk, float* __restrict__ partial) {
    __shared__ f32x4 red[2][8][32];
    const int cq = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 128 + cq * 4, C = L.C, R = L.N * L.B;
    const bool cok = c < C;
    f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    if (cok) {
        const f32x4 mu = *(const f32x4*)(mean + c), is = *(const f32x4*)(invstd + c);
        const int l0 = blockIdx.y * rows_per_chunk, l1 = l0 + rows_per_chunk < R ? l0 + rows_per_chunk : R;
        for (int l = l0; l < l1; ++l) {
            if (!ct_row_valid(L, l)) continue;
            const long long o = (long long)l * L.P1 * C + c;
            for (int p = rl; p < L.P1; p += 8) {
                const long long e = o + (long long)p * C;
                f32x4 gv = *(const f32x4*)(g + e);
                if (RELU) {
                    const f32x4 yv = *(const f32x4*)(y + e);
#pragma unroll
                    for (int j = 0; j < 4; ++j) gv[j] = yv[j] > 0.f ? gv[j] : 0.f;
                }
                const f32x4 xh = (*(const f32x4*)(x + e) - mu) * is;
                s0 += gv; s1 += gv * xh;
            }
        }
    }
    red[0][rl][cq] = s0; red[1][rl][cq] = s1;
    __syncthreads();
    if (rl == 0 && cok) {
#pragma unroll
        for (int i = 1; i < 8; ++i) { s0 += red[0][i][cq]; s1 += red[1][i][cq]; }
        float* dst = partial + (long long)blockIdx.y * 2 * C;
        *(f32x4*)(dst + c) = s0;
        *(f32x4*)(dst + C + c) = s1;
    }
}

__global__ __launch_bounds__(256) void afi_roi_bn_bwd_finalize_kernel(const float* __restrict__ partial, int chunks, int C,
                                                                      float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                      float* __restrict__ sums) {
    __shared__ float red[2][8][CT_FIN_CH];
    const int cl = threadIdx.x & (CT_FIN_CH - 1), ln = threadIdx.x / CT_FIN_CH;
    const int c = blockIdx.x * CT_FIN_CH + cl;
    float a0 = 0.f, a1 = 0.f;
    if (c < C)
        for (int i = ln; i < chunks; i += 8) { a0 += partial[(long long)i * 2 * C + c]; a1 += partial[(long long)i * 2 * C + C + c]; }
    red[0][ln][cl] = a0; red[1][ln][cl] = a1;
    __syncthreads();
    if (ln != 0 || c >= C) return;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { s0 += red[0][j][cl]; s1 += red[1][j][cl]; }
    sums[c] = s0; sums[C + c] = s1;
    if (dbeta) dbeta[c] += s0;
    if (dgamma) dgamma[c] += s1;
}

// One list row per block at a time (grid-stride over the N B rows); its P1 C / 4 float4 items over the 256 threads.  With 256 % (C / 4) == 0 a
// thread stays on one channel quad and its parameter vectors are loaded once.
// BWD = false: y = relu((x - mean) invstd gamma + beta) (afi_bn_affine) on valid rows, 0 on padding rows.
// BWD = true:  dx = gamma invstd (g' - s0 / Pn - xhat s1 / Pn) on valid rows, 0 on padding rows (dx may be g: neither is __restrict__).
template <bool BWD, bool RELU>
__global__ __launch_bounds__(256) void afi_roi_bn_apply_kernel(const float* g, const float* __restrict__ x, const float* __restrict__ y,
                                                               const CtList L, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ sums, float* out) {
    const int C = L.C, C4 = C >> 2, R = L.N * L.B, items = L.P1 * C4, tid = threadIdx.x;
    const bool hoist = (256 % C4) == 0;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    float inv_n = 0.f;
    if (BWD) {
        const long long Pn = ct_valid_rows(L, nullptr) * L.P1;
        inv_n = Pn > 0 ? 1.f / (float)Pn : 0.f;
    }
    f32x4 mu = zero, is = zero, ga = zero, be = zero, sg = zero, sgx = zero;
    auto params = [&](int c) {
        mu = *(const f32x4*)(mean + c); is = *(const f32x4*)(invstd + c); ga = *(const f32x4*)(gamma + c);
        if (BWD) { sg = *(const f32x4*)(sums + c); sgx = *(const f32x4*)(sums + C + c); }
        else be = *(const f32x4*)(beta + c);
    };
    if (hoist) params((tid % C4) * 4);
    for (int l = blockIdx.x; l < R; l += gridDim.x) {
        const long long o = (long long)l * items * 4;
        if (!ct_row_valid(L, l)) {
            for (int e = tid; e < items; e += 256) *(f32x4*)(out + o + (long long)e * 4) = zero;
            continue;
        }
        for (int e = tid; e < items; e += 256) {
            if (!hoist) params((e % C4) * 4);
            const long long a = o + (long long)e * 4;
            const f32x4 xv = __builtin_nontemporal_load((const f32x4*)(x + a));
            f32x4 r;
            if (BWD) {
                f32x4 gv = *(const f32x4*)(g + a);
                if (RELU) {
                    const f32x4 yv = __builtin_nontemporal_load((const f32x4*)(y + a));
#pragma unroll
                    for (int j = 0; j < 4; ++j) gv[j] = yv[j] > 0.f ? gv[j] : 0.f;
                }
                const f32x4 xh = (xv - mu) * is;
                r = ga * is * (gv - sg * inv_n - xh * (sgx * inv_n));
            } else {
                r = afi_bn_affine(xv, mu, is, ga, be);
                if (RELU) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) r[j] = r[j] > 0.f ? r[j] : 0.f;
                }
            }
            *(f32x4*)(out + a) = r;
        }
    }
}

static int ct_list_ok(const int* counts, int N, int B, int P1, int C) {
    if (!counts || N <= 0 || B <= 0 || P1 <= 0 || C <= 0 || (C & 3)) return AFI_ERR_BAD_ARG;
    if (N > CT_MAX_N || B > CT_MAX_B || (long long)N * B * P1 * (C >> 2) > 0x7fffffffll) return AFI_ERR_UNSUPPORTED;     // the 32-bit row and item indices
    return AFI_OK;
}
// chunks of LIST rows: as many as afi_red_geometry would cut the N B P1 pixel rows into, but never less than one list row each
static void ct_red_geometry(int R, int P1, int& chunks, int& rows_per_chunk) {
    long long want = ((long long)R * P1 + 63) / 64;
    if (want > CT_RED_MAX_CHUNKS) want = CT_RED_MAX_CHUNKS;
    if (want > R) want = R;
    if (want < 1) want = 1;
    rows_per_chunk = (int)((R + want - 1) / want);
    chunks = (R + rows_per_chunk - 1) / rows_per_chunk;
}
static unsigned ct_ew_grid(int R) { return (unsigned)(R > CT_EW_GRID_CAP ? CT_EW_GRID_CAP : R); }

extern "C" int afi_roi_bn_stats(const float* x, const int* counts, int N, int B, int P1, int C, float eps, float momentum, float* mean,
                                float* invstd, float* var_biased_or_null, float* running_mean_or_null, float* running_var_or_null,
                                long long* num_batches_tracked_or_null, float* scratch, void* stream) {
    AFI_TRY(ct_list_ok(counts, N, B, P1, C));
    if (!x || !mean || !invstd || !scratch || !(eps >= 0.f) || (running_mean_or_null == nullptr) != (running_var_or_null == nullptr))
        return AFI_ERR_BAD_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)scratch & 31)) return AFI_ERR_UNSUPPORTED;
    const CtList L{counts, N, B, P1, C};
    int chunks, rpc;
    ct_red_geometry(N * B, P1, chunks, rpc);
    hipLaunchKernelGGL(afi_roi_bn_stats_partial_kernel, dim3(afi_cdiv(C, 128), chunks), dim3(256), 0, (hipStream_t)stream, x, L, rpc, (double*)scratch);
    hipLaunchKernelGGL(afi_roi_bn_stats_finalize_kernel, dim3(afi_cdiv(C, CT_FIN_CH)), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, chunks,
                       x, L, mean, invstd, var_biased_or_null, running_mean_or_null, running_var_or_null, num_batches_tracked_or_null, eps, momentum);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

extern "C" int afi_roi_bn_relu_fwd(const float* x, const int* counts, int N, int B, int P1, int C, const float* mean, const float* invstd,
                                   const float* gamma, const float* beta, int relu, float* y, void* stream) {
    AFI_TRY(ct_list_ok(counts, N, B, P1, C));
    if (!x || !mean || !invstd || !gamma || !beta || !y || (relu != 0 && relu != 1)) return AFI_ERR_BAD_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)mean & 15) || ((uintptr_t)invstd & 15) || ((uintptr_t)gamma & 15) ||
        ((uintptr_t)beta & 15))
        return AFI_ERR_UNSUPPORTED;
    const CtList L{counts, N, B, P1, C};
    const dim3 grid(ct_ew_grid(N * B));
    if (relu) hipLaunchKernelGGL((afi_roi_bn_apply_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, (const float*)nullptr, x, (const float*)nullptr, L, mean, invstd, gamma, beta, (const float*)nullptr, y);
    else hipLaunchKernelGGL((afi_roi_bn_apply_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, (const float*)nullptr, x, (const float*)nullptr, L, mean, invstd, gamma, beta, (const float*)nullptr, y);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

extern "C" int afi_roi_bn_relu_bwd_sums(const float* g, const float* x, const float* y_or_null, const int* counts, int N, int B, int P1, int C,
                                        const float* mean, const float* invstd, int relu, float* dgamma_or_null, float* dbeta_or_null,
                                        float* sums2C, float* scratch, void* stream) {
    AFI_TRY(ct_list_ok(counts, N, B, P1, C));
    if (!g || !x || !mean || !invstd || !sums2C || !scratch || (relu != 0 && relu != 1) || (relu && !y_or_null)) return AFI_ERR_BAD_ARG;
    if (((uintptr_t)g & 15) || ((uintptr_t)x & 15) || ((uintptr_t)y_or_null & 15) || ((uintptr_t)mean & 15) || ((uintptr_t)invstd & 15) ||
        ((uintptr_t)scratch & 15))
        return AFI_ERR_UNSUPPORTED;
    const CtList L{counts, N, B, P1, C};
    int chunks, rpc;
    ct_red_geometry(N * B, P1, chunks, rpc);
    const dim3 grid(afi_cdiv(C, 128), chunks);
    if (relu) hipLaunchKernelGGL(afi_roi_bn_bwd_partial_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g, x, y_or_null, L, mean, invstd, rpc, scratch);
    else hipLaunchKernelGGL(afi_roi_bn_bwd_partial_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, g, x, (const float*)nullptr, L, mean, invstd, rpc, scratch);
    hipLaunchKernelGGL(afi_roi_bn_bwd_finalize_kernel, dim3(afi_cdiv(C, CT_FIN_CH)), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, chunks, C,
                       dgamma_or_null, dbeta_or_null, sums2C);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

extern "C" int afi_roi_bn_relu_bwd_apply(const float* g, const float* x, const float* y_or_null, const int* counts, int N, int B, int P1, int C,
                                         const float* mean, const float* invstd, const float* gamma, const float* sums2C, int relu, float* dx,
                                         void* stream) {
    AFI_TRY(ct_list_ok(counts, N, B, P1, C));
    if (!g || !x || !mean || !invstd || !gamma || !sums2C || !dx || (relu != 0 && relu != 1) || (relu && !y_or_null)) return AFI_ERR_BAD_ARG;
    if (((uintptr_t)g & 15) || ((uintptr_t)x & 15) || ((uintptr_t)y_or_null & 15) || ((uintptr_t)dx & 15) || ((uintptr_t)mean & 15) ||
        ((uintptr_t)invstd & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)sums2C & 15))
        return AFI_ERR_UNSUPPORTED;
    const CtList L{counts, N, B, P1, C};
    const dim3 grid(ct_ew_grid(N * B));
    if (relu) hipLaunchKernelGGL((afi_roi_bn_apply_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, g, x, y_or_null, L, mean, invstd, gamma, (const float*)nullptr, sums2C, dx);
    else hipLaunchKernelGGL((afi_roi_bn_apply_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, g, x, (const float*)nullptr, L, mean, invstd, gamma, (const float*)nullptr, sums2C, dx);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
