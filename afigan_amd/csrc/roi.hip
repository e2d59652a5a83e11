// The box branch of the frozen StandardROIHeads (afigan_amd/roi_heads.py): detectron2 v0.1.1's ROIPooler / ROIAlignV2 (aligned) and
// fast_rcnn_inference.  The box head's FCs and the predictor between the two run on afi_conv1x1_fwd over the R = N P rows as pixels.
//   afi_roi_align         multi-level ROIAlign of a padded [N][P][4] box list into [N P][S][S][C].  One wave per (roi, bin group): lanes run
//                         across channels with 16-byte loads (at C = 256 one pixel's channels are one coalesced 1 KiB wave load); with fewer
//                         than 64 float4 per pixel a wave takes 64 / (C / 4) bins of the same roi.  Level, grid, sample coordinates and the
//                         four bilinear weights are evaluated in fp64 from the fp32 box, operation by operation (no contraction), and never
//                         stored: every discrete decision (level, grid, inside test, y_low) is the formula's own.  The weights are rounded to
//                         fp32 and the samples summed in fp32 in (iy, ix, corner) order.  No LDS, no atomics.
//   afi_roi_scores_boxes  one wave per row: softmax over the K + 1 logits in fp64 (fixed butterfly order), Box2BoxTransform.apply_deltas
//                         + clip per class in fp64, each rounded once.
//   afi_roi_cascade_stage the same row code with class-agnostic boxes, the score added to the previous stages' running score and, at the last
//                         stage, scaled by 1 / S (CascadeROIHeads): one launch per stage, the per-stage scores are never stored.
//   afi_roi_candidates    afi_rpn_topk on the scores seen as a [N][P][K][1] map (index r K + c), then per candidate class, box, valid and the
//                         count of all scores above the threshold (a fixed-order block sum).
//   afi_roi_nms           afi_select.h's greedy NMS with classes.
//   afi_roi_pick          the first D kept candidates by a block prefix sum; the truncated flag.
// Nothing here synchronises with the host, and every result is bit-identical from run to run and under hipGraph replay.
#include "../../include/afigan_hip.h"
#include "afi_common.h"
#include "afi_select.h"
#include "afi_roi_decode.h"

#define ROI_MAX_LEVELS 8
#define ROI_MAX_S 14
#define ROI_MAX_GRID 4096          // samples per bin and axis: a box of more than 4096 S level pixels per side is sampled on this grid
#define ROI_MAX_K 1024
#define ROI_CANON_SIZE 224.0
#define ROI_CANON_LEVEL 4.0

struct RoiLevels {
    int L, min_level;
    AfiView v[ROI_MAX_LEVELS];
    int H[ROI_MAX_LEVELS], W[ROI_MAX_LEVELS];
};

// ------------------------------------------------------------------------------------------------ ROIAlign
// G: bins per wave (1 when C4 >= 64, else min(64 / C4, S S)); gpr = ceil(S S / G) bin groups per roi.
__global__ __launch_bounds__(256) void afi_roi_align_kernel(const RoiLevels lv, int N, int P, int C4, int S, int sr, int G, int gpr,
                                                            const float* __restrict__ boxes, const int* __restrict__ counts,
                                                            float* __restrict__ out) {
#pragma clang fp contract(off)                          // the geometry is the stated fp64 expression, operation by operation; the sums use fmaf
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long grp = (long long)blockIdx.x * 4 + wave, total = (long long)N * P * gpr;
    if (grp >= total) return;
    const long long roi = grp / gpr;
    const int g = (int)(grp - roi * gpr), n = (int)(roi / P), j = (int)(roi - (long long)n * P);
    const int sub = C4 >= 64 ? 0 : lane / C4, c0 = C4 >= 64 ? lane : lane - sub * C4;
    const int bin = g * G + sub;
    if (sub >= G || bin >= S * S) return;
    float4* o = (float4*)out + (roi * S * S + bin) * C4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* b = boxes + 4 * roi;
    const double x1 = (double)b[0], y1 = (double)b[1], x2 = (double)b[2], y2 = (double)b[3];
    const double bw = x2 - x1, bh = y2 - y1;
    if (j >= counts[n] || !(bw > 0.0 && bh > 0.0)) {      // padding rows; a non-positive (or NaN) side: no samples, zeros
        for (int c = c0; c < C4; c += 64) o[c] = zero;
        return;
    }
    const double lf = floor(ROI_CANON_LEVEL + log2(sqrt(bw * bh) / ROI_CANON_SIZE));
    int level = lv.min_level;
    if (lf > (double)lv.min_level) level = lf < (double)(lv.min_level + lv.L - 1) ? (int)lf : lv.min_level + lv.L - 1;
    const int li = __builtin_amdgcn_readfirstlane(level - lv.min_level);       // one roi per wave: uniform
    const int H = lv.H[li], W = lv.W[li];
    const AfiView v = lv.v[li];
    const double scale = 1.0 / (double)(1 << level);
    const double sw = x1 * scale - 0.5, sh = y1 * scale - 0.5, rw = bw * scale, rh = bh * scale;
    const double binw = rw / (double)S, binh = rh / (double)S;
    int gh = sr, gw = sr;
    if (sr <= 0) {
        const double a = ceil(rh / (double)S), c = ceil(rw / (double)S);
        gh = a < (double)ROI_MAX_GRID ? (int)a : ROI_MAX_GRID;
        gw = c < (double)ROI_MAX_GRID ? (int)c : ROI_MAX_GRID;
    }
    const int cnt = gh * gw > 1 ? gh * gw : 1;
    const int ph = bin / S, pw = bin - ph * S;
    const float* base = v.p + (long long)n * v.sN;
    for (int c = c0; c < C4; c += 64) {
        float4 acc = zero;
        for (int iy = 0; iy < gh; ++iy) {
            double y = sh + (double)ph * binh + ((double)iy + 0.5) * binh / (double)gh;
            if (y < -1.0 || y > (double)H) continue;
            if (y <= 0.0) y = 0.0;
            int yl = (int)y, yh;
            if (yl >= H - 1) { yl = yh = H - 1; y = (double)yl; } else yh = yl + 1;
            const double ly = y - (double)yl, hy = 1.0 - ly;
            const float* r0 = base + (long long)yl * v.sH + 4 * c;
            const float* r1 = base + (long long)yh * v.sH + 4 * c;
            for (int ix = 0; ix < gw; ++ix) {
                double x = sw + (double)pw * binw + ((double)ix + 0.5) * binw / (double)gw;
                if (x < -1.0 || x > (double)W) continue;
                if (x <= 0.0) x = 0.0;
                int xl = (int)x, xh;
                if (xl >= W - 1) { xl = xh = W - 1; x = (double)xl; } else xh = xl + 1;
                const double lx = x - (double)xl, hx = 1.0 - lx;
                const float w1 = (float)(hy * hx), w2 = (float)(hy * lx), w3 = (float)(ly * hx), w4 = (float)(ly * lx);
                const float4 f1 = *(const float4*)(r0 + (long long)xl * v.sW), f2 = *(const float4*)(r0 + (long long)xh * v.sW);
                const float4 f3 = *(const float4*)(r1 + (long long)xl * v.sW), f4 = *(const float4*)(r1 + (long long)xh * v.sW);
                acc.x = fmaf(w4, f4.x, fmaf(w3, f3.x, fmaf(w2, f2.x, fmaf(w1, f1.x, acc.x))));
                acc.y = fmaf(w4, f4.y, fmaf(w3, f3.y, fmaf(w2, f2.y, fmaf(w1, f1.y, acc.y))));
                acc.z = fmaf(w4, f4.z, fmaf(w3, f3.z, fmaf(w2, f2.z, fmaf(w1, f1.z, acc.z))));
                acc.w = fmaf(w4, f4.w, fmaf(w3, f3.w, fmaf(w2, f2.w, fmaf(w1, f1.w, acc.w))));
            }
        }
        const float fc = (float)cnt;
        o[c] = make_float4(acc.x / fc, acc.y / fc, acc.z / fc, acc.w / fc);
    }
}

int afi_roi_align(const afi_view_t* levels, const int* level_hw, int L, int min_level, int N, int C, const float* boxes, const int* counts, int P,
                  int S, int sampling_ratio, float* out, void* stream) {
    if (!levels || !level_hw || !boxes || !counts || !out || L <= 0 || min_level < 0 || N <= 0 || N > 65535 || C <= 0 || P <= 0 || S <= 0 ||
        sampling_ratio < 0)
        return AFI_ERR_BAD_ARG;
    if (L > ROI_MAX_LEVELS || min_level + L - 1 > 30 || (C & 3) || S > ROI_MAX_S || sampling_ratio > ROI_MAX_GRID || ((uintptr_t)out & 15) ||
        ((uintptr_t)boxes & 3))
        return AFI_ERR_UNSUPPORTED;
    RoiLevels lv;
    lv.L = L;
    lv.min_level = min_level;
    for (int l = 0; l < ROI_MAX_LEVELS; ++l) {
        const int s = l < L ? l : L - 1;
        const afi_view_t& q = levels[s];
        if (!q.p || level_hw[2 * s] <= 0 || level_hw[2 * s + 1] <= 0) return AFI_ERR_BAD_ARG;
        if (((uintptr_t)q.p & 15) || (q.sN & 3) || (q.sH & 3) || (q.sW & 3)) return AFI_ERR_UNSUPPORTED;
        lv.v[l] = AfiView{q.p, q.sN, q.sH, q.sW};
        lv.H[l] = level_hw[2 * s];
        lv.W[l] = level_hw[2 * s + 1];
    }
    const int C4 = C / 4, SS = S * S;
    int G = 1;
    if (C4 < 64) { G = 64 / C4; if (G > SS) G = SS; }
    const int gpr = (SS + G - 1) / G;
    const long long blocks = ((long long)N * P * gpr + 3) / 4;
    if (blocks > 0x7fffffffll) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_roi_align_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, lv, N, P, C4, S, sampling_ratio, G, gpr,
                       boxes, counts, out);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ scores and boxes
// (RoiDecode, the softmax / decode row code roi_scores_boxes_row and its helpers: afi_roi_decode.h, shared with cascade_train.hip)

__global__ __launch_bounds__(256) void afi_roi_scores_boxes_kernel(const RoiDecode d, const float* __restrict__ pred,
                                                                   const float* __restrict__ proposals, const int* __restrict__ counts,
                                                                   const float* __restrict__ image_hw, float* __restrict__ scores,
                                                                   float* __restrict__ boxes) {
    roi_scores_boxes_row<false>(d, pred, proposals, counts, image_hw, nullptr, 1.f, scores, boxes);
}

// (scores and prev_scores may be one buffer: neither is __restrict__)
__global__ __launch_bounds__(256) void afi_roi_cascade_stage_kernel(const RoiDecode d, const float* __restrict__ pred,
                                                                    const float* __restrict__ proposals, const int* __restrict__ counts,
                                                                    const float* __restrict__ image_hw, const float* prev_scores, float out_scale,
                                                                    float* scores, float* __restrict__ boxes) {
    roi_scores_boxes_row<true>(d, pred, proposals, counts, image_hw, prev_scores, out_scale, scores, boxes);
}

int afi_roi_scores_boxes(const float* pred, long long ld_pred, int N, int P, int K, int agnostic, const float* proposals, const int* counts,
                         const float* image_hw, float wx, float wy, float ww, float wh, double scale_clamp, float* scores, float* boxes,
                         void* stream) {
    if (!pred || !proposals || !counts || !image_hw || !scores || !boxes || N <= 0 || N > 65535 || P <= 0 || K <= 0 ||
        (agnostic != 0 && agnostic != 1))
        return AFI_ERR_BAD_ARG;
    if (K > ROI_MAX_K) return AFI_ERR_UNSUPPORTED;
    if (ld_pred < (long long)K + 1 + 4 * (agnostic ? 1 : K)) return AFI_ERR_BAD_ARG;
    if (!(wx > 0.f) || !(wy > 0.f) || !(ww > 0.f) || !(wh > 0.f)) return AFI_ERR_BAD_ARG;
    const RoiDecode d{N, P, K, agnostic, ld_pred, wx, wy, ww, wh, scale_clamp};
    const long long blocks = ((long long)N * P + 3) / 4;
    if (blocks > 0x7fffffffll) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_roi_scores_boxes_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d, pred, proposals, counts, image_hw,
                       scores, boxes);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

int afi_roi_cascade_stage(const float* pred, long long ld_pred, int N, int P, int K, const float* proposals, const int* counts,
                          const float* image_hw, float wx, float wy, float ww, float wh, double scale_clamp, const float* prev_scores,
                          float out_scale, float* scores, float* boxes, void* stream) {
    if (!pred || !proposals || !counts || !image_hw || !scores || !boxes || N <= 0 || N > 65535 || P <= 0 || K <= 0) return AFI_ERR_BAD_ARG;
    if (K > ROI_MAX_K) return AFI_ERR_UNSUPPORTED;
    if (ld_pred < (long long)K + 1 + 4) return AFI_ERR_BAD_ARG;
    if (!(wx > 0.f) || !(wy > 0.f) || !(ww > 0.f) || !(wh > 0.f) || !(out_scale > 0.f) || out_scale > 3.4e38f) return AFI_ERR_BAD_ARG;
    const RoiDecode d{N, P, K, 1, ld_pred, wx, wy, ww, wh, scale_clamp};
    const long long blocks = ((long long)N * P + 3) / 4;
    if (blocks > 0x7fffffffll) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_roi_cascade_stage_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d, pred, proposals, counts, image_hw,
                       prev_scores, out_scale, scores, boxes);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ candidates
// One block per image, after afi_rpn_topk has written cand_scores / cand_idx [img][0 .. m).
__global__ __launch_bounds__(1024) void afi_roi_cand_kernel(const float* __restrict__ scores, const float* __restrict__ boxes, int P, int K, int Kb,
                                                            float thresh, int m, int M, float* __restrict__ cs, int* __restrict__ ci,
                                                            float* __restrict__ cb, int* __restrict__ cc, int* __restrict__ cv,
                                                            int* __restrict__ n_over) {
    __shared__ int wtot[16];
    const int img = blockIdx.x, tid = threadIdx.x, n = P * K;
    const float* s = scores + (long long)img * n;
    int cnt = 0;
    for (int i = tid; i < n; i += 1024) cnt += s[i] > thresh ? 1 : 0;
    int total;
    rpn_block_scan(cnt, wtot, &total);
    if (tid == 0) n_over[img] = total;
    if (tid >= M) return;
    const long long o = (long long)img * M + tid;
    float sv = -INFINITY, x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    int idx = -1, cls = -1, ok = 0;
    if (tid < m) {
        const int i = ci[o];
        if (i >= 0 && i < n) {                         // (always: afi_rpn_topk's indices)
            const int r = i / K, c = i - r * K;
            const float* q = boxes + 4 * ((long long)img * P * Kb + (long long)r * Kb + (Kb == 1 ? 0 : c));
            sv = cs[o]; idx = i; cls = c;
            x1 = q[0]; y1 = q[1]; x2 = q[2]; y2 = q[3];
            ok = sv > thresh;
        }
    }
    cs[o] = sv; ci[o] = idx; cc[o] = cls; cv[o] = ok;
    float* p = cb + 4 * o;
    p[0] = x1; p[1] = y1; p[2] = x2; p[3] = y2;
}

long long afi_roi_candidates_ws_floats(int N, int P, int K) {
    if (N <= 0 || P <= 0 || K <= 0 || K > ROI_MAX_K || (long long)P * K >= 0x3FFFFF) return -1;
    return afi_rpn_topk_ws_floats(N, P, K, 1);
}

int afi_roi_candidates(const float* scores, const float* boxes, int N, int P, int K, int agnostic, float score_thresh, int M, float* cand_scores,
                       int* cand_idx, float* cand_boxes, int* cand_cls, int* cand_valid, int* n_over, float* ws, long long ws_floats,
                       void* stream) {
    if (!scores || !boxes || !cand_scores || !cand_idx || !cand_boxes || !cand_cls || !cand_valid || !n_over || N <= 0 || N > 65535 || P <= 0 ||
        K <= 0 || M <= 0 || (agnostic != 0 && agnostic != 1))
        return AFI_ERR_BAD_ARG;
    if (K > ROI_MAX_K || M > RPN_MAXK || (long long)P * K >= 0x3FFFFF) return AFI_ERR_UNSUPPORTED;
    const int n = P * K, m = M < n ? M : n;
    // the scores as a [N][P][K][1] map: "anchor" index (y W + x) A + a = r K + c
    const afi_view_t v{(float*)scores, (long long)n, (long long)K, 1};
    const int st = afi_rpn_topk(v, N, P, K, 1, m, cand_scores, cand_idx, M, ws, ws_floats, stream);
    if (st != AFI_OK) return st;
    hipLaunchKernelGGL(afi_roi_cand_kernel, dim3(N), dim3(1024), 0, (hipStream_t)stream, scores, boxes, P, K, agnostic ? 1 : K, score_thresh, m, M,
                       cand_scores, cand_idx, cand_boxes, cand_cls, cand_valid, n_over);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ NMS with classes
int afi_roi_nms(const float* boxes, const int* cls, const int* valid, int N, int k, long long ld, float thresh, int* keep, void* stream) {
    if (N <= 0 || N > 65535 || k < 0 || ld < k) return AFI_ERR_BAD_ARG;
    if (k == 0) return AFI_OK;
    if (!boxes || !cls || !valid || !keep) return AFI_ERR_BAD_ARG;
    if (k > RPN_MAXK) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_nms_kernel<true>, dim3(N), dim3(1024), 0, (hipStream_t)stream, boxes, cls, valid, k, ld, thresh, keep);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ pick
__global__ __launch_bounds__(1024) void afi_roi_pick_kernel(const float* __restrict__ cb, const float* __restrict__ cs, const int* __restrict__ cc,
                                                            const int* __restrict__ keep, const int* __restrict__ n_over, int M, int D,
                                                            float* __restrict__ ob, float* __restrict__ os, int* __restrict__ oc,
                                                            int* __restrict__ counts, int* __restrict__ truncated) {
    __shared__ int wtot[16];
    const int img = blockIdx.x, tid = threadIdx.x;
    const long long src = (long long)img * M + tid;
    const int f = tid < M && keep[src] != 0;
    int total;
    const int pos = rpn_block_scan(f, wtot, &total) - 1;
    const int c = total < D ? total : D;
    if (f && pos < D) {
        const long long dst = (long long)img * D + pos;
        const float* q = cb + 4 * src;
        float* p = ob + 4 * dst;
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; p[3] = q[3];
        os[dst] = cs[src];
        oc[dst] = cc[src];
    }
    if (tid >= c && tid < D) {
        const long long dst = (long long)img * D + tid;
        float* p = ob + 4 * dst;
        p[0] = 0.f; p[1] = 0.f; p[2] = 0.f; p[3] = 0.f;
        os[dst] = 0.f;
        oc[dst] = 0;
    }
    if (tid == 0) {
        counts[img] = c;
        truncated[img] = (n_over[img] > M && total < D) ? 1 : 0;
    }
}

int afi_roi_pick(const float* cand_boxes, const float* cand_scores, const int* cand_cls, const int* keep, const int* n_over, int N, int M, int D,
                 float* out_boxes, float* out_scores, int* out_classes, int* counts, int* truncated, void* stream) {
    if (!cand_boxes || !cand_scores || !cand_cls || !keep || !n_over || !out_boxes || !out_scores || !out_classes || !counts || !truncated ||
        N <= 0 || N > 65535 || M <= 0 || D <= 0)
        return AFI_ERR_BAD_ARG;
    if (M > RPN_MAXK || D > RPN_MAXK) return AFI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(afi_roi_pick_kernel, dim3(N), dim3(1024), 0, (hipStream_t)stream, cand_boxes, cand_scores, cand_cls, keep, n_over, M, D,
                       out_boxes, out_scores, out_classes, counts, truncated);
    return hipGetLastError() == hipSuccess ? AFI_OK : AFI_ERR_LAUNCH;
}
