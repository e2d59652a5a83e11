// The row code of afi_roi_scores_boxes / afi_roi_cascade_stage (roi.hip) as device functions, so that every kernel that decodes a predictor row
// evaluates ONE definition: the softmax over the K + 1 logits and Box2BoxTransform.apply_deltas + clip, both in fp64 from the fp32 inputs and
// rounded once.  csrc/cascade_train.hip decodes the next stage's training boxes with roi_decode_clip, the function roi_scores_boxes_row calls.
#pragma once
#include "afi_common.h"

struct RoiDecode {
    int N, P, K, agnostic;
    long long ld;
    float wx, wy, ww, wh;
    double clamp;
};

__device__ __forceinline__ double roi_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double roi_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The running score of the cascade: (prev + s) and then, when out_scale != 1, the product with out_scale -- one fp32 operation each.
__device__ __forceinline__ float roi_running_score(float s, const float* prev, float out_scale) {
#pragma clang fp contract(off)
    float v = prev ? *prev + s : s;               // (the lane reads its own element before it writes it: scores may be prev_scores)
    if (out_scale != 1.f) v = v * out_scale;
    return v;
}

// A proposal (x1, y1, x2, y2) as apply_deltas reads it: width, height and centre in fp64.
struct RoiBoxGeom { double w, h, cx, cy; };
__device__ __forceinline__ RoiBoxGeom roi_box_geom(const float* p) {
    const double px1 = (double)p[0], py1 = (double)p[1], px2 = (double)p[2], py2 = (double)p[3];
    RoiBoxGeom g;
    g.w = px2 - px1;
    g.h = py2 - py1;
    g.cx = px1 + 0.5 * g.w;
    g.cy = py1 + 0.5 * g.h;
    return g;
}

// o[0..4) = clip(apply_deltas(t[0..4) / weights, proposal), image): dw / dh clamped from above at d.clamp, every coordinate rounded to fp32
// once and clipped to [0, iw] / [0, ih] in fp32 (fmaxf / fminf: a NaN coordinate clips to 0).
__device__ __forceinline__ void roi_decode_clip(const RoiDecode& d, const float* t, const RoiBoxGeom& b, float ih, float iw, float* o) {
    const double dx = (double)t[0] / (double)d.wx, dy = (double)t[1] / (double)d.wy;
    const double dw = fmin((double)t[2] / (double)d.ww, d.clamp), dh = fmin((double)t[3] / (double)d.wh, d.clamp);
    const double pcx = dx * b.w + b.cx, pcy = dy * b.h + b.cy, pw = exp(dw) * b.w, ph = exp(dh) * b.h;
    o[0] = fminf(fmaxf((float)(pcx - 0.5 * pw), 0.f), iw);
    o[1] = fminf(fmaxf((float)(pcy - 0.5 * ph), 0.f), ih);
    o[2] = fminf(fmaxf((float)(pcx + 0.5 * pw), 0.f), iw);
    o[3] = fminf(fmaxf((float)(pcy + 0.5 * ph), 0.f), ih);
}

// One wave per row r = n P + j; lane c, c + 64, ...: class c.  CASCADE: the scores go through roi_running_score (d.agnostic is 1 there).
template <bool CASCADE>
__device__ __forceinline__ void roi_scores_boxes_row(const RoiDecode& d, const float* pred, const float* proposals, const int* counts,
                                                     const float* image_hw, const float* prev, float out_scale, float* scores, float* boxes) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)d.N * d.P) return;
    const int n = (int)(row / d.P), j = (int)(row - (long long)n * d.P), K = d.K, Kb = d.agnostic ? 1 : K;
    float* sc = scores + row * K;
    float* bx = boxes + row * Kb * 4;
    const float* pv = CASCADE && prev ? prev + row * K : nullptr;
    if (j >= counts[n]) {
        for (int c = lane; c < K; c += 64) sc[c] = CASCADE ? roi_running_score(-INFINITY, pv ? pv + c : nullptr, out_scale) : -INFINITY;
        for (int c = lane; c < 4 * Kb; c += 64) bx[c] = 0.f;
        return;
    }
    const float* q = pred + row * d.ld;
    double m = -INFINITY;
    bool bad = false;
    for (int c = lane; c <= K; c += 64) {
        const float l = q[c];
        bad |= l != l;
        m = fmax(m, (double)l);
    }
    m = roi_wave_max(m);
    bad = __any(bad);
    double s = 0.0;
    for (int c = lane; c <= K; c += 64) s += exp((double)q[c] - m);
    s = roi_wave_sum(s);
    const RoiBoxGeom g = roi_box_geom(proposals + 4 * row);
    const float ih = image_hw[2 * n], iw = image_hw[2 * n + 1];
    const float* dl = q + K + 1;
    for (int c = lane; c < K; c += 64) {
        const float sv = bad ? __builtin_nanf("") : (float)(exp((double)q[c] - m) / s);
        sc[c] = CASCADE ? roi_running_score(sv, pv ? pv + c : nullptr, out_scale) : sv;
        if (c < Kb) roi_decode_clip(d, dl + 4 * c, g, ih, iw, bx + 4 * c);
    }
}
