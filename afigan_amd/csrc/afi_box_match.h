// detectron2's pairwise_iou and Matcher as device functions over boxes held in registers or LDS, whatever they were read from: the RPN's label
// assignment (rpn_loss.hip: anchors formed from their index, ground truth from a padded tensor) and the ROI heads' proposal labelling (roi_loss.hip).
// Every operation is rounded to fp32 once and nothing is contracted into a fused multiply-add, as in rpn_overlaps (afi_select.h): an IoU
// computed here is the same bit pattern wherever it is computed, so two sweeps may compare their results for equality.
#pragma once
#include "afi_common.h"

__device__ __forceinline__ float afi_box_area(const float4 b) {
#pragma clang fp contract(off)
    return (b.z - b.x) * (b.w - b.y);
}

// inter > 0 ? inter / (area_a + area_b - inter) : 0, with w = max(min(x2) - max(x1), 0) and h likewise.  Never -0, never negative.
__device__ __forceinline__ float afi_box_iou(const float4 a, const float area_a, const float4 b, const float area_b) {
#pragma clang fp contract(off)
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f), h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
    const float inter = w * h;
    return inter > 0.f ? inter / (area_a + area_b - inter) : 0.f;
}

// Matcher over one candidate: the running (maximum IoU, lowest ground-truth index that reaches it).  Start from {0.f, 0}: a candidate that
// overlaps nothing is matched to box 0 with value 0, as max over a column of zeros gives.
struct AfiMatch { float val; int idx; };
__device__ __forceinline__ void afi_match_update(AfiMatch& m, const float iou, const int g) {
    if (iou > m.val) { m.val = iou; m.idx = g; }
}

// Matcher's thresholds with labels [0, -1, 1]: 0 below t0, -1 (ignored) in [t0, t1), 1 from t1 up.
__device__ __forceinline__ int afi_match_label(const float val, const float t0, const float t1) { return val < t0 ? 0 : (val < t1 ? -1 : 1); }
